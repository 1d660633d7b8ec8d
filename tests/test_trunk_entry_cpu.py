"""The seven entry points of cz_conv.hip without a GPU: a NULL context is refused with CZ_EINVAL before anything else is
touched, and cz_last_error() holds the entry's own text, byte for byte."""
import pytest

EINVAL = -1
# entry point -> (arguments behind the context, the text of the refusal)
NULL_CONTEXT = {
    "cz_conv3x3_c128_bf16": ((None, None, None, None, None, 0, 0), b"cz_conv3x3_c128_bf16: null argument"),
    "cz_tower_c128_bf16": ((None, None, None, None, 0, 1), b"cz_tower_c128_bf16: null argument / nblocks < 1"),
    "cz_tower_heads_c128_bf16": ((None,) * 7 + (0, 1), b"cz_tower_heads_c128_bf16: null argument / nblocks < 1"),
    "cz_net_trunk_bf16": ((None,) * 9 + (0, 1), b"cz_net_trunk_bf16: null argument / nblocks < 1"),
    "cz_net_trunk_f16": ((None,) * 9 + (0, 1), b"cz_net_trunk_f16: null argument / nblocks < 1"),
    "cz_net_trunk_split": ((None,) * 9 + (0, 1, 2), b"cz_net_trunk_split: null argument / nblocks < 1"),
    "cz_net_trunk_mx": ((None,) * 9 + (0, 1), b"cz_net_trunk_mx: null argument / nblocks < 1"),
}


@pytest.fixture(scope="module", autouse=True)
def _library():
    import __graft_entry__
    __graft_entry__.build_hip_only()


@pytest.mark.parametrize("name", sorted(NULL_CONTEXT))
def test_a_null_context_is_refused_by_name(name):
    from cchess_zero_amd import _lib
    L = _lib.lib()
    args, text = NULL_CONTEXT[name]
    assert len(args) + 1 == len(_lib._SIGS[name][1])
    assert getattr(L, name)(None, *args) == EINVAL
    assert L.cz_last_error() == text
