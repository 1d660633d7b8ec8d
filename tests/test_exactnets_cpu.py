"""The exact tier's own proof obligations, without a GPU (tests/exactnets.py): for every case tests/test_net_exact.py runs on the
MI355X, "the kernel must equal the float64 reference bit for bit" is a theorem (check_exact: stored values survive their
format, every partial sum is an exact fp32 number, the net is alive), the reference agrees exactly with the fp32 torch module
and with the NumPy restatement of the reference graph, and every deliberate corruption of the reference (a swapped tap, channel
or position, a wrapped border, a missing residual, a dropped lo half, a wrong block scale) changes the expected outputs.
The round families, whose activations are off every engine's storage grid, also show here that the reference's explicit storage
step meets every rounding, saturation and scale case of its list in every kind of layer, that each corruption of that step
changes the expected outputs, and that the explicit step leaves every other family's expected outputs bit for bit as they were."""
import numpy as np
import pytest
import torch

import exactnets as E
import mxemu
from cchess_zero_amd.net import PolicyValueModule
from oracle import net_numpy

_CASES = sorted({(f, b, s, e) for e, cs in E.CASES.items() for f, b, seeds in cs for s in seeds})
_modules = {}


def _module(family, blocks, seed, half=torch.float16):
    key = (family, blocks, seed, half if family in ("lo", "round", "round_x2") else torch.float16)
    if key not in _modules:
        _modules[key] = E.build(PolicyValueModule(blocks), family, seed, key[3])
    return _modules[key]


@pytest.mark.parametrize("family,blocks,seed,engine", _CASES)
def test_check_exact_holds_for_every_gpu_case(family, blocks, seed, engine):
    """conditions (a), (b) and (c) on every batch the GPU test feeds this engine (exactnets.gpu_batches: the 93 rows, the pairs
    and dense rows of its small batches — a batch of 5 holds the batches of 1, 2 and 3 as prefixes, rows are independent — and
    the 64 dense rows), and on their union: every output channel of every layer is non-zero somewhere, so that no entry of a
    packed weight image is only ever multiplied by zero on the GPU"""
    m = _module(family, blocks, seed, E.HALF[engine])
    alive = None
    for name, x in E.gpu_batches(engine).items():
        r = E.check_exact(m, x, engine, liveness=name == "live")
        alive = r["channels_alive"] if alive is None else alive | r["channels_alive"]
        print("%s %s x %d seed %d, %s rows: largest activation %.6g, largest sum %.3g of 2^24 granules, %d (layer, channel) pairs alive" %
              (engine, family, blocks, seed, name, r["max_activation"], r["max_sum_over_2^24g"], int(r["channels_alive"].sum())))
    assert alive.shape == (2 * blocks + 1, 128) and bool(alive.all()), "dead (layer, channel) pairs on the GPU's rows: %s" % (~alive).nonzero().tolist()


@pytest.mark.parametrize("engine", sorted(E.ROUND_SEEDS))
def test_round_family_meets_every_storage_case(engine):
    """counted on the float64 reference alone, over the engine's 1- and 2-block round nets and every batch the GPU test feeds them:
    at least 32 elements of every case of exactnets.round_cases in EVERY kind of layer that stores (first conv,
    first and second conv of a block); mx6: 24 distinct activation scale bytes.  Condition (b) holds element by element
    (check_exact; the largest sum / 2^24 g is printed)"""
    tally, ratio = {}, 0.0
    for blocks, seed in zip((1, 2), E.ROUND_SEEDS[engine]):
        m = _module(E.ROUND_FAMILY[engine], blocks, seed, E.HALF[engine])
        for name, x in E.gpu_batches(engine).items():
            E.reference(m, x, engine, tally=tally)
            ratio = max(ratio, E.check_exact(m, x, engine, liveness=False)["max_sum_over_2^24g"])
    print("%s: largest sum / 2^24 g %.3g" % (engine, ratio))
    for case in E.round_cases(engine):
        per_kind = [tally.get((k, case), 0) for k in E.ROUND_KINDS]
        print("%s %-18s %s" % (engine, case, "  ".join("%s: %d" % kc for kc in zip(E.ROUND_KINDS, per_kind))))
        assert min(per_kind) >= 32, (engine, case, per_kind)
    if engine == "mx6":
        print("mx6: %d distinct activation scale bytes: %s" % (len(tally["bytes"]), sorted(tally["bytes"])))
        assert len(tally["bytes"]) >= 24 and 1 in tally["bytes"]
    assert ratio < 1.0


@pytest.mark.parametrize("family,blocks,seed,engine", [c for c in _CASES if c[0] not in E.ROUND_FAMILIES])
def test_explicit_storage_step_leaves_the_other_families_unchanged(family, blocks, seed, engine):
    """the storage step the round families go through is the identity on every other case: the expected outputs with the step
    forced on equal, bit for bit, those of the path without it (the clamp alone, what this reference always computed)"""
    m = _module(family, blocks, seed, E.HALF[engine])
    for name, x in E.gpu_batches(engine).items():
        if name == "dense":
            continue                               # (its rows are the first five of "live")
        old, new = E.reference(m, x, engine, storage="identity"), E.reference(m, x, engine, storage="explicit")
        plain = E.reference(m, x, engine)
        for k in ("trunk", "z", "logits"):
            assert torch.equal(old[k], new[k]) and torch.equal(old[k], plain[k]), (name, k)
        assert all(torch.equal(a, b) for a, b in zip(old["layers"], new["layers"]))


def test_dense_family_covers_every_tower_weight_entry():
    cover = None
    for seed in range(E.DENSE_SEEDS):
        nz = torch.stack([cb.folded()[0] != 0 for blk in _module("dense", 1, seed).blocks for cb in blk])
        cover = nz if cover is None else cover | nz
    assert cover.shape == (2, 128, 128, 3, 3) and bool(cover.all())
    for fam in ("sparse", "lo", "mx_cross"):      # every tap and every input channel of every layer is used
        for cb in (c for blk in _module(fam, 2 if fam != "sparse" else 3, 0).blocks for c in blk):
            nz = cb.folded()[0] != 0
            assert bool(nz.any(0).any(0).all()) and bool(nz.any(0).any(-1).any(-1).all()), fam


@pytest.mark.parametrize("family,blocks", [("sparse", 1), ("sparse", 3), ("sparse", 7), ("dense", 1)])
def test_fp32_torch_module_equals_float64_reference(family, blocks):
    """PolicyValueModule.forward (unfolded BN, fp32: the graph every engine is measured against) == the float64 reference of
    the folded graph, exactly: trunk activations and both head convs"""
    m = _module(family, blocks, 0)
    x = E.batch93()
    got = {}
    h1 = m.policy_conv.register_forward_pre_hook(lambda mod, inp: got.__setitem__("trunk", inp[0].detach()))
    h2 = m.policy_conv.register_forward_hook(lambda mod, inp, out: got.__setitem__("p", out.detach()))
    h3 = m.value_conv.register_forward_hook(lambda mod, inp, out: got.__setitem__("v", out.detach()))
    try:
        with torch.no_grad():
            m(x.permute(0, 3, 1, 2).contiguous())
    finally:
        for h in (h1, h2, h3):
            h.remove()
    ref = E.reference(m, x, "fp16")
    trunk = got["trunk"].permute(0, 2, 3, 1).reshape(93, 90, 128)
    z = torch.relu(torch.cat([got["p"], got["v"]], 1)).permute(0, 2, 3, 1).reshape(93, 90, 3)
    assert E.describe_mismatch(trunk, ref["trunk"], "fp32 module trunk", x) is None
    assert E.describe_mismatch(z, ref["z"], "fp32 module head convs", x) is None


@pytest.mark.parametrize("blocks", [1, 3])
def test_numpy_restatement_equals_float64_reference_on_sparse(blocks):
    """oracle.net_numpy.forward — what north_star's 1e-3 is stated against — gives the float64 graph's logits exactly on the
    sparse family (its policy FC sums are exact fp32 numbers too: asserted)"""
    m = _module("sparse", blocks, 0)
    x = torch.cat([E.planes("impulses")[::9], E.planes("dense", 8)])
    ref = E.reference(m, x, "fp16")
    p = ref["z"][:, :, :2].reshape(x.shape[0], 180)
    w, b = m.policy_fc.weight.detach().double(), m.policy_fc.bias.detach().double()
    assert float((p.abs() @ w.abs().t() + b.abs()).max()) < 2.0 ** 24 * 2.0 ** -12      # granule of w, b: 2^-12; p: integers
    logits = p @ w.t() + b
    ln, _ = net_numpy.forward(m.export_tf_layout(), x.numpy(), blocks)
    assert ln.dtype == np.float32 and np.array_equal(ln.astype(np.float64), logits.numpy())


def test_mx_reference_is_mxemu_in_float64():
    """the layer-by-layer mx6 reference (it needs the per-layer activations and the hooks of MUTATIONS) is
    mxemu.forward_mx(dtype=float64); the float32 default of mxemu is what it was"""
    x = torch.cat([E.planes("impulses")[::9], E.planes("dense", 3)])
    for fam, blocks, seed in (("mx_cross", 2, 1), ("sparse", 3, 0), ("lo", 1, 0)):
        m = _module(fam, blocks, seed)
        ref = E.reference(m, x, "mx6")
        with torch.no_grad():
            lg, _, v = mxemu.forward_mx(m, x.permute(0, 3, 1, 2).contiguous(), dtype=torch.float64)
            l32, _, v32 = mxemu.forward_mx(m, x.permute(0, 3, 1, 2).contiguous())
        assert v.dtype == torch.float64 and torch.equal(v, ref["layers"][-1])
        assert v32.dtype == torch.float32 and l32.dtype == torch.float32 and torch.equal(v32.double(), v)
        p = ref["z"][:, :, :2].reshape(x.shape[0], 180)
        assert torch.equal(lg, p @ m.policy_fc.weight.detach().double().t() + m.policy_fc.bias.detach().double())


@pytest.mark.parametrize("family,blocks,seed,engine", _CASES)
def test_every_mutation_changes_the_expected_outputs(family, blocks, seed, engine):
    """the suite's sensitivity, for every case and seed: each applicable corruption of the reference changes the trunk output
    and the head convs on rows of the 93-row batch (every 15th impulse + the dense rows; rows are independent, pos_swap pairs
    neighbours of this sub-batch).  The corrupted layer is the second conv of the first block and, in the deeper nets, also
    that of the last but one block"""
    m = _module(family, blocks, seed, E.HALF[engine])
    x = torch.cat([E.planes("impulses")[::15], E.planes("dense", 3)])
    ref = E.reference(m, x, engine)
    names = E.applicable_mutations(family, engine, x.shape[0])
    assert len(names) >= 6 and ("lo_zero" in names) == (family in ("lo", "lo_subnormal", "mx_cross", "round_x2", "round_mx"))
    assert ("scale_off" in names) == (family in ("mx_cross", "round_mx"))
    rnd = family in E.ROUND_FAMILIES
    assert [n for n in E._STORE_MUTATIONS if n in names] == ([n for n, es in E._STORE_MUTATIONS.items() if engine in es] if rnd else [])
    for layer in ([1] if blocks < 3 else [1, 2 * blocks - 3]):
        for name in names:
            if layer > 1 and name in ("lo_zero", "scale_off"):
                continue                                   # these corrupt the layer that carries w_lo, whatever `layer`
            mut = E.reference(m, x, engine, mutation=name, mut_layer=layer)
            nt, nz = int((mut["trunk"] != ref["trunk"]).sum()), int((mut["z"] != ref["z"]).sum())
            print("%s %s x %d seed %d, layer %d, %s (%s): %d trunk values and %d head conv outputs change" %
                  (engine, family, blocks, seed, layer, name, E.MUTATIONS[name][0], nt, nz))
            if rnd:        # (its head convs read six channels, of three classes: the trunk output or z must change)
                assert nt + nz > 0, "%s in layer %d changes nothing: the inputs are too weak" % (name, layer)
                continue
            assert nt > 0, "%s in layer %d changes nothing: the inputs are too weak" % (name, layer)
            assert nz > 0, "%s in layer %d does not reach the head convs" % (name, layer)


def test_three_term_reference_stays_within_its_dropped_term_bound():
    """strict engines on values with lo halves: the plain float64 graph differs from the three-term reference (the a_lo w_lo
    products are dropped) by no more than the bound the reference returns, and does differ"""
    x = E.batch93()
    for engine, fam, blocks in (("fp16x2", "lo", 2), ("bf16x2", "lo", 2), ("fp16x2", "lo_subnormal", 1)):
        m = _module(fam, blocks, 0, E.HALF[engine])
        three, plain = E.reference(m, x, engine), E.reference(m, x, "fp16" if fam == "lo_subnormal" else "layer")
        d = (plain["trunk"] - three["trunk"]).abs()
        # (these nets are all-positive: the bound is attained, and the plain graph's own lo x lo x lo terms need more than
        # float64's 53 bits at the last layer, hence the 2^-30 relative slack on a comparison of two float64 evaluations)
        assert bool((d <= three["trunk_bound"] * (1.0 + 2.0 ** -30)).all()) and float(d.max()) > 0.0
        assert float(three["trunk_bound"].max()) < 2.0 ** -16 * float(three["trunk"].max())


def test_layer_kernel_and_fc_inputs_are_provably_exact():
    """the inputs tests/test_net_exact.py feeds the per-layer bf16 kernels and the policy FC meet conditions (a) and (b)"""
    x, res = E.layer_activations(5, 0.3, 3), torch.roll(E.layer_activations(6, 0.3, 3), 1, 0)
    for seed in range(E.DENSE_SEEDS):
        for cb in _module("dense", 1, seed).blocks[0]:
            w, b = cb.folded()
            for r, relu in ((None, True), (res, True), (res, False), (None, False)):
                assert not E.conv_layer_check(x, w, b, r, relu)
    x, res, off = E.conv_layer_rounding_inputs()          # the same kernel where its two roundings are NOT the identity
    for seed in range(E.DENSE_SEEDS):
        for cb in _module("dense", 1, seed).blocks[0]:
            w, b = cb.folded()
            for r, relu in ((None, True), (res, True), (res, False), (None, False)):
                assert not E.conv_layer_check(x, w, b + off, r, relu, rounding=True)
    for blocks in (1, 3):
        out = E.tower_reference(_module("sparse", blocks, 0), E.layer_activations(7, 0.25, 3), "layer", check=True)
        assert float((out["trunk"] != 0).double().mean()) > 0.1 and float((out["z"] != 0).double().mean()) > 0.1
        assert all(bool(((v != 0).sum(dim=(0, 2, 3)) > 0).all()) for v in out["layers"])      # every channel of every layer is alive
    # the round family through the per-layer route (two roundings per residual layer) and through the fused tower (one): exact, and different
    m = _module("round", 1, E.ROUND_SEEDS["bf16"][0], torch.bfloat16)
    fused = E.reference(m, E.batch93(), "bf16")
    out = E.tower_reference(m, fused["layers"][0].permute(0, 2, 3, 1).reshape(93, 90, 128), "layer", check=True)
    assert int((out["trunk"] != fused["trunk"]).sum()) >= 32
    for B in (5, 129):
        z = E.fc_inputs(B)
        assert not E.fc_check(_module("sparse", 1, 0), z)
        p = z[:, :, :2].reshape(B, 180).double()       # the dropped z_lo w_lo products are there: the three-term sum is not the plain one
        plain = p @ _module("sparse", 1, 0).policy_fc.weight.detach().double().t() + _module("sparse", 1, 0).policy_fc.bias.detach().double()
        assert not torch.equal(plain, E.fc_reference(_module("sparse", 1, 0), z))


def test_prefix_net_hands_out_layer_2k():
    """layer localisation of the GPU test: a k-block net on the first k blocks of the same weights has layer 2k as trunk output"""
    m = _module("sparse", 3, 0)
    x = torch.cat([E.planes("impulses")[::30], E.planes("dense", 2)])
    ref = E.reference(m, x, "fp16")
    for k in (1, 2):
        pk = E.reference(E.prefix_module(m, k), x, "fp16")
        assert torch.equal(pk["layers"][-1], ref["layers"][2 * k]) and len(pk["layers"]) == 2 * k + 1
    for engine in sorted(E.ROUND_SEEDS):                     # ... under every engine's storage step too (round family, 2 blocks)
        m = _module(E.ROUND_FAMILY[engine], 2, E.ROUND_SEEDS[engine][1], E.HALF[engine])
        ref, pk = E.reference(m, x, engine), E.reference(E.prefix_module(m, 1), x, engine)
        assert torch.equal(pk["layers"][-1], ref["layers"][2]) and len(pk["layers"]) == 3
    cells = E.impulse_cells(E.planes("pairs", 5, group=4))
    assert (cells >= 0).tolist() == [True, False, True, False, False] and int(cells[2]) == 14
    assert (E.impulse_cells(E.planes("pairs", 5, group=2)) >= 0).tolist() == [True, False, False, True, True]


def test_describe_mismatch_names_the_coordinate():
    x = E.batch93()
    ref = torch.zeros(93, 90, 128)
    got = ref.clone()
    got[37, 46, 5] = 2.0
    msg = E.describe_mismatch(got, ref, "fp16x2 sparse x 3 trunk", x, group=2)
    assert "row 37 (position 2 of 2" in msg and "y 4, x 6, channel 5" in msg and "got 2.0, expected 0.0" in msg
    assert "1 of " in msg and "(dy, dx) = (+1, -1)" in msg
    assert E.describe_mismatch(-ref, ref, "signed zero") is None
    got[0, 0, 0] = float("nan")
    assert "row 0" in E.describe_mismatch(got, ref, "nan")
