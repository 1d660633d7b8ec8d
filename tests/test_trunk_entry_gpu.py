"""The six one-launch trunk entry points of cz_conv.hip on one context: what each refuses on the host, in front of any launch, with
its exact text; B = 0; and one valid launch at the smallest ragged batch on a 1-block net, repeated on the same context (the
second launch takes the path behind the dynamic-LDS opt-in) with the same output.  The values themselves: test_net_exact.py."""
import pytest
import torch

pytestmark = pytest.mark.gpu

OK, EINVAL = 0, -1
F16, BF16 = 2, 1
# entry -> (net, positions per workgroup + 1 = the smallest ragged batch, the name its alignment errors carry)
ENTRIES = {
    "cz_tower_c128_bf16": ("bf16", 5, None),
    "cz_tower_heads_c128_bf16": ("bf16", 5, "cz_net_trunk"),
    "cz_net_trunk_bf16": ("bf16", 5, "cz_net_trunk"),
    "cz_net_trunk_f16": ("f16", 5, "cz_net_trunk"),
    "cz_net_trunk_split": ("split", 3, "cz_net_trunk_split"),
    "cz_net_trunk_mx": ("mx", 3, "cz_net_trunk_mx"),
}
HEADS = [e for e in ENTRIES if e != "cz_tower_c128_bf16"]


class Rig:
    def __init__(self):
        from cchess_zero_amd.engine import Context
        from cchess_zero_amd.net import PolicyValueModule, PolicyValueNet
        self.ctx = Context(1, 2, 0)
        m = PolicyValueModule(1, 0)
        kw = dict(res_block_nums=1, device="cuda:0", module=m, backend="hip", ctx=self.ctx)
        self.nets = {"bf16": PolicyValueNet(dtype=torch.bfloat16, **kw), "f16": PolicyValueNet(dtype=torch.float16, **kw),
                     "split": PolicyValueNet(dtype=torch.float16, split=True, **kw), "mx": PolicyValueNet(dtype=torch.float16, split="mx", **kw)}
        g = torch.Generator().manual_seed(5)
        self.planes = torch.zeros((5, 9, 10, 16))
        self.planes[..., :14] = (torch.rand((5, 9, 10, 14), generator=g) > 0.8).float()
        self.acts = torch.rand((5, 90, 128), generator=g)
        self.keep = []

    def args(self, entry, B, nblocks=1, head_w="net", head_out="z", wpk="net", halves=F16):
        """-> (the arguments behind the context, the output tensor)"""
        net = self.nets[ENTRIES[entry][0]]
        hdt = torch.bfloat16 if net.dtype == torch.bfloat16 else torch.float16
        n = max(B, 1)
        z = torch.zeros((n, 90, 3), dtype=torch.float32, device="cuda:0")
        head_w = net.head_w_rows if head_w == "net" else head_w
        head_out = z if head_out == "z" else head_out
        if entry.startswith("cz_tower"):
            x = self.acts[:n].to("cuda:0").to(hdt).contiguous()
            if entry == "cz_tower_c128_bf16":
                return (x, net.hip_tower_w, net.hip_tower_b, x, B, nblocks), x
            return (x, net.hip_tower_w, net.hip_tower_b, None, head_w, net.head_b, head_out, B, nblocks), z
        p16 = self.planes[:n].to("cuda:0").to(hdt).contiguous()
        w0, w = {"cz_net_trunk_split": ("hip_split_w0", "hip_split_w"), "cz_net_trunk_mx": ("hip_split_w0", "hip_mx_w")}.get(entry, ("hip_w0", "hip_tower_w"))
        a = (p16, getattr(net, w0), net.hip_b0, getattr(net, w) if wpk == "net" else wpk, net.hip_tower_b, None, head_w, net.head_b, head_out, B, nblocks)
        return a + ((halves,) if entry == "cz_net_trunk_split" else ()), z

    def raw(self, entry, a):
        """the entry on the context, unchecked -> (return code, cz_last_error())"""
        from cchess_zero_amd import _lib
        self.ctx.bind_stream()
        self.keep.append(a)
        rc = getattr(_lib.lib(), entry)(self.ctx.h, *[x.data_ptr() if hasattr(x, "data_ptr") else x for x in a])
        return rc, _lib.lib().cz_last_error()


@pytest.fixture(scope="module")
def rig():
    r = Rig()
    yield r
    torch.cuda.synchronize()
    r.ctx.close()


@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_nblocks_0_is_refused(rig, entry):
    a, _ = rig.args(entry, ENTRIES[entry][1], nblocks=0)
    assert rig.raw(entry, a) == (EINVAL, b"%s: null argument / nblocks < 1" % entry.encode())


@pytest.mark.parametrize("entry", HEADS)
def test_head_out_without_head_w_is_refused(rig, entry):
    a, _ = rig.args(entry, ENTRIES[entry][1], head_w=None)
    text = b"cz_tower_heads_c128_bf16: null argument / nblocks < 1" if entry == "cz_tower_heads_c128_bf16" else b"%s: head_out needs head_w and head_b" % entry.encode()
    assert rig.raw(entry, a) == (EINVAL, text)


@pytest.mark.parametrize("entry", HEADS)
def test_a_misaligned_head_w_is_refused(rig, entry):
    off = torch.zeros(3 * 128 + 4, dtype=torch.float32, device="cuda:0")[1:1 + 3 * 128]
    assert off.data_ptr() % 16 == 4
    a, _ = rig.args(entry, ENTRIES[entry][1], head_w=off)
    assert rig.raw(entry, a) == (EINVAL, b"%s: head_w must be 16-byte aligned" % ENTRIES[entry][2].encode())


def test_misaligned_mx_weights_are_refused(rig):
    w = rig.nets["mx"].hip_mx_w
    off = torch.zeros(w.numel() + 16, dtype=torch.uint8, device="cuda:0")[8:8 + w.numel()]
    assert off.data_ptr() % 16 == 8
    a, _ = rig.args("cz_net_trunk_mx", 3, wpk=off)
    assert rig.raw("cz_net_trunk_mx", a) == (EINVAL, b"cz_net_trunk_mx: wpk must be 16-byte aligned")


@pytest.mark.parametrize("halves", [0, 3])
def test_split_refuses_another_halves_dtype(rig, halves):
    assert (F16, BF16) == (2, 1)
    a, _ = rig.args("cz_net_trunk_split", 3, halves=halves)
    assert rig.raw("cz_net_trunk_split", a) == (EINVAL, b"cz_net_trunk_split: halves_dtype must be CZ_F16 or CZ_BF16")


@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_an_empty_batch_is_ok(rig, entry):
    a, _ = rig.args(entry, 0)
    assert rig.raw(entry, a)[0] == OK


@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_a_ragged_batch_twice_on_one_context(rig, entry):
    B = ENTRIES[entry][1]
    outs = []
    for _ in range(2):
        a, out = rig.args(entry, B)
        assert rig.raw(entry, a)[0] == OK
        torch.cuda.synchronize()
        outs.append(out.float().cpu())
    assert torch.isfinite(outs[0]).all() and float(outs[0].abs().max()) > 0
    assert torch.equal(outs[0], outs[1])
