"""Exact-arithmetic conformance of every net trunk kernel (GPU).  The nets of tests/exactnets.py have weights and activations of
so few significant bits that every partial sum of every conv is an exact fp32 number (tests/test_exactnets_cpu.py proves it for
each case below): whatever the tiling, the MFMA shape and the order of the additions, the kernel must reproduce the float64
reference BIT FOR BIT.  Every comparison of a kernel's output with its reference is equality of values (+0 == -0, no NaN): no
kernel is held to a tolerance in this file.  (One inequality between two float64 evaluations — the plain graph against the
three-term reference's dropped-term bound — carries a relative 2^-30 for float64's own rounding of the plain graph.)  A
failure names the engine, the family, the depth, the first differing (row, y, x, channel), got / expected, how many elements
differ, for an impulse row the (dy, dx) offset from the impulse, and the row's place in its workgroup; for the deeper nets also the
first layer that differs.  The value head goes through tanh and is not asserted here (test_net.py::test_hip_fc_heads_vs_fp64)."""
import ctypes as C

import pytest
import torch

import exactnets as E

pytestmark = pytest.mark.gpu

_SPLIT = {"bf16": False, "fp16": False, "bf16x2": True, "fp16x2": True, "mx6": "mx"}
_refs = {}


def _module(family, blocks, seed, half):
    from cchess_zero_amd.net import PolicyValueModule
    return E.build(PolicyValueModule(blocks).to("cuda:0"), family, seed, half)


def _net(module, engine):
    from cchess_zero_amd.net import PolicyValueNet
    net = PolicyValueNet(module.res_block_nums, "cuda:0", E.HALF[engine], module=module, split=_SPLIT[engine])
    assert net.backend == "hip" and net.engine_name == engine
    return net


def _reference(module, family, blocks, seed, engine, xname, x):
    """computed once per (net, reference engine, batch) and shared by the engines it serves; never modified"""
    ref_engine = E.reference_engine(family, engine)
    key = (family, blocks, seed, E.HALF[engine] if family == "lo" else None, ref_engine, xname)
    if key not in _refs:
        _refs[key] = E.reference(module, x, ref_engine)
    return _refs[key]


def _run(net, x):
    """-> (trunk [B,90,128] from repacked f32 planes, z [B,90,3] from zero-copy 16-channel planes in the operand type)"""
    xd = x.cuda()
    x16 = torch.zeros((x.shape[0], 9, 10, 16), dtype=net.dtype, device="cuda")
    x16[..., :14] = xd.to(net.dtype)
    trunk = net._hip_net_forward(xd, trunk=True)
    z = net._hip_net_forward(x16)
    if net.dtype == torch.float16 or net.split:    # the public route to the same kernel for fp16 and the strict engines
        assert torch.equal(net.tower(xd).permute(0, 2, 3, 1).reshape(trunk.shape), trunk)
    torch.cuda.synchronize()
    return trunk, z


def _first_bad_layer(module, family, seed, engine, x, ref):
    """a k-block net on the first k blocks of the same weights hands out layer 2k as its trunk output"""
    for k in range(1, module.res_block_nums):
        net = _net(E.prefix_module(module, k), engine)
        got = net._hip_net_forward(x.cuda(), trunk=True)
        if engine == "mx6":      # (a prefix net writes layer 2k as fp32 after a ReLU alone; the full net clamps it at 65504 when it stores it)
            got = got.clamp(max=65504.0)
        exp = ref["layers"][2 * k].permute(0, 2, 3, 1).reshape(got.shape)
        if E.describe_mismatch(got, exp, "") is not None:
            return "; the first layer that differs is %d or %d (the %d-block prefix net)" % (2 * k - 1, 2 * k, k)
    return "; every shorter prefix net is exact: the last block differs"


def _compare(net, module, family, blocks, seed, engine, xname, x):
    ref = _reference(module, family, blocks, seed, engine, xname, x)
    trunk, z = _run(net, x)
    what = "%s %s x %d seed %d, %s rows" % (engine, family, blocks, seed, xname)
    msg = E.describe_mismatch(trunk, ref["trunk"], what + ", trunk output", x, E.GROUP[engine])
    if msg is not None and blocks > 1:
        msg += _first_bad_layer(module, family, seed, engine, x, ref)
    assert msg is None, msg
    msg = E.describe_mismatch(z, ref["z"], what + ", head conv outputs z", x, E.GROUP[engine])
    assert msg is None, msg
    return ref, trunk


@pytest.mark.parametrize("engine,family,blocks", [(e, f, b) for e in sorted(E.CASES) for f, b, _ in E.CASES[e]])
def test_trunk_kernel_is_bit_exact(engine, family, blocks):
    """k_tower8_c128 (bf16, fp16), k_trunk_split_c128 (bf16x2, fp16x2), k_trunk_mx_c128 (mx6): trunk output and head conv
    outputs on the 93 rows (90 impulses, one per cell + 3 dense: a last workgroup with one live position) and on batches of 1,
    2, 3 and 5 rows of impulses whose workgroup partners are dense, and of dense rows, and on 64 dense rows."""
    g = E.GROUP[engine]
    seeds = [s for f, b, s in E.CASES[engine] if (f, b) == (family, blocks)][0]
    for seed in seeds:
        module = _module(family, blocks, seed, E.HALF[engine])
        net = _net(module, engine)
        ref, trunk = _compare(net, module, family, blocks, seed, engine, "93", E.batch93())
        if family in ("lo", "lo_subnormal"):
            # the kernel equals the three-term reference (above); the plain float64 graph is within the dropped a_lo w_lo bound
            plain = _reference(module, family, blocks, seed, "layer" if engine == "bf16x2" else "fp16", "93", E.batch93())
            d = (plain["trunk"] - trunk.cpu().double()).abs()
            assert bool((d <= ref["trunk_bound"] * (1.0 + 2.0 ** -30)).all())      # (2^-30: float64 rounding of the plain graph's own lo x lo terms)
        batches = E.gpu_batches(engine)
        assert len(batches) == 4
        # the 64 dense rows: with them every output channel of every layer is non-zero somewhere (test_exactnets_cpu.py), so
        # every entry of every packed weight image meets a non-zero activation
        _compare(net, module, family, blocks, seed, engine, "live", batches.pop("live"))
        batches.pop("93")
        for kind, xs in batches.items():
            for B in E.SMALL_B:
                _compare(net, module, family, blocks, seed, engine, "%s[:%d]" % (kind, B), xs[:B])


@pytest.mark.parametrize("engine", sorted(E.CASES))
def test_trunk_kernel_is_bit_exact_under_the_device_row_count(engine):
    """the compact path (cz_set_batch_count): 11 of the 93 rows are computed, and they are the reference's bits"""
    _row_count_case(engine, "sparse", 0)


@pytest.mark.parametrize("engine", sorted(E.CASES))
def test_round_trunk_kernel_is_bit_exact_under_the_device_row_count(engine):
    """the same on the round family (1 block): the storage step of every layer under the device-side row count"""
    _row_count_case(engine, E.ROUND_FAMILY[engine], E.ROUND_SEEDS[engine][0])


def _row_count_case(engine, family, seed):
    from cchess_zero_amd._lib import check, lib
    module = _module(family, 1, seed, E.HALF[engine])
    net = _net(module, engine)
    x = E.batch93()
    ref = _reference(module, family, 1, seed, engine, "93", x)
    n = torch.tensor([11], dtype=torch.int32, device="cuda")
    check(lib().cz_set_batch_count(net._hip_ctx().h, C.c_void_p(n.data_ptr())), "cz_set_batch_count")
    try:
        trunk = net._hip_net_forward(x.cuda(), trunk=True)[:11].clone()
        z = net._hip_net_forward(x.cuda())[:11].clone()
        torch.cuda.synchronize()
    finally:
        check(lib().cz_set_batch_count(net._hip_ctx().h, None), "cz_set_batch_count")
    what = "%s %s x 1, 11 of 93 rows by the device-side row count" % (engine, family)
    msg = E.describe_mismatch(trunk, ref["trunk"][:11], what + ", trunk output", x[:11], E.GROUP[engine])
    assert msg is None, msg
    msg = E.describe_mismatch(z, ref["z"][:11], what + ", head conv outputs z", x[:11], E.GROUP[engine])
    assert msg is None, msg


def _impulse_note(x, r):
    nz = x[r].nonzero()
    return " (row %d is an impulse at y %d, x %d, channel %d)" % (r, nz[0, 0] // 10, nz[0, 0] % 10, nz[0, 1]) if nz.shape[0] == 1 else ""


@pytest.mark.parametrize("residual,relu", [(False, True), (True, True), (True, False), (False, False)])
def test_conv3x3_layer_kernel_is_bit_exact(residual, relu):
    """cz_conv3x3_c128_bf16 on the dense family (every weight entry non-zero in one of its seeds): integer activations fed
    directly, residual on / off, ReLU on / off.  The kernel rounds to bf16 before the residual add: the reference's pre-residual
    sums and results are asserted to be bf16 values, so that rounding is the identity."""
    _conv3x3_case(residual, relu, False)


@pytest.mark.parametrize("residual,relu", [(False, True), (True, True), (True, False), (False, False)])
def test_conv3x3_layer_kernel_rounds_to_nearest_even(residual, relu):
    """the same kernel on activations up to 40 and biases with eighths, for which neither its rounding before the residual add nor
    its final rounding is the identity: the reference states both, and exactnets.conv_layer_check counts at least 32 values
    rounded down, 32 rounded up and 32 exact ties on each"""
    _conv3x3_case(residual, relu, True)


def _conv3x3_case(residual, relu, rounding):
    from cchess_zero_amd.net import PolicyValueNet
    if rounding:
        x, res, off = E.conv_layer_rounding_inputs()
    else:
        x, res, off = E.layer_activations(5, 0.3, 3), torch.roll(E.layer_activations(6, 0.3, 3), 1, 0), torch.zeros(128)
    res = res if residual else None
    for seed in range(E.DENSE_SEEDS):
        module = _module("dense", 1, seed, torch.bfloat16)
        net = PolicyValueNet(1, "cuda:0", torch.bfloat16, module=module, backend="hip-layer")
        for li, cb in enumerate(module.blocks[0]):
            w, b = cb.folded()
            b = b.cpu() + off
            exp = E.conv_layer_reference(x, w, b, res, relu)[0]
            assert not E.conv_layer_check(x, w, b, res, relu, rounding)
            out = torch.full((x.shape[0], 90, 128), float("nan"), device="cuda", dtype=torch.bfloat16)
            wp, bp = net.hip_blocks[0][li]
            assert bp.dtype == torch.float32 and torch.equal(bp.cpu(), cb.folded()[1].cpu())
            net._hip_conv(x.cuda().to(torch.bfloat16), (wp, b.float().cuda().contiguous()), res.cuda().to(torch.bfloat16) if residual else None, out, relu)
            torch.cuda.synchronize()
            msg = E.describe_mismatch(out, exp, "cz_conv3x3_c128_bf16 dense seed %d layer %d residual %s relu %s rounding %s" % (seed, li, residual, relu, rounding))
            assert msg is None, msg + _impulse_note(x, int(msg.split("first at row ")[1].split(" ")[0]))


@pytest.mark.parametrize("blocks", [1, 3])
def test_tower_layer_kernels_are_bit_exact(blocks):
    """cz_tower_c128_bf16 (tower output) and cz_tower_heads_c128_bf16 (z) on the sparse family, and the per-layer route
    (cz_conv3x3_c128_bf16 block by block), integer activations fed directly"""
    from cchess_zero_amd.net import PolicyValueNet
    module = _module("sparse", blocks, 0, torch.bfloat16)
    net = PolicyValueNet(blocks, "cuda:0", torch.bfloat16, module=module, backend="hip-layer")
    x = E.layer_activations(7, 0.25, 3)
    ref = E.tower_reference(module, x, "layer", check=True)
    h = x.cuda().to(torch.bfloat16).reshape(-1, 9, 10, 128).permute(0, 3, 1, 2)          # [B,128,9,10] channels_last
    got = net._hip_tower_forward(h.clone(memory_format=torch.channels_last)).permute(0, 2, 3, 1).reshape(x.shape)
    z = net._hip_tower_heads_forward(h.clone(memory_format=torch.channels_last))
    per_layer = net._hip_blocks_forward(h.clone(memory_format=torch.channels_last)).permute(0, 2, 3, 1).reshape(x.shape)
    torch.cuda.synchronize()
    for name, g, e in (("cz_tower_c128_bf16 tower output", got, ref["trunk"]), ("cz_tower_heads_c128_bf16 z", z, ref["z"]),
                       ("cz_conv3x3_c128_bf16 layer by layer", per_layer, ref["trunk"])):
        msg = E.describe_mismatch(g, e, "%s, sparse x %d" % (name, blocks))
        assert msg is None, msg + _impulse_note(x, int(msg.split("first at row ")[1].split(" ")[0]))


def test_tower_layer_kernels_round_to_nearest_even():
    """the same three routes on the round family (bf16, 1 block), fed the reference's stored first-conv activations of the 93
    rows: no rounding is the identity here.  cz_tower_c128_bf16 / cz_tower_heads_c128_bf16 add the residual in fp32 and round
    once (the bf16 engine's reference); cz_conv3x3_c128_bf16 block by block rounds before the residual add and again after it
    (the "layer" reference, whose conditions of exactness are asserted) — and the two references differ"""
    from cchess_zero_amd.net import PolicyValueNet
    seed = E.ROUND_SEEDS["bf16"][0]
    module = _module("round", 1, seed, torch.bfloat16)
    net = PolicyValueNet(1, "cuda:0", torch.bfloat16, module=module, backend="hip-layer")
    fused = _reference(module, "round", 1, seed, "bf16", "93", E.batch93())
    x = fused["layers"][0].permute(0, 2, 3, 1).reshape(93, 90, 128)
    assert torch.equal(x.float().to(torch.bfloat16).double(), x)
    ref = E.tower_reference(module, x, "layer", check=True)
    assert int((ref["trunk"] != fused["trunk"]).sum()) >= 32
    h = x.float().cuda().to(torch.bfloat16).reshape(-1, 9, 10, 128).permute(0, 3, 1, 2)
    got = net._hip_tower_forward(h.clone(memory_format=torch.channels_last)).permute(0, 2, 3, 1).reshape(x.shape)
    z = net._hip_tower_heads_forward(h.clone(memory_format=torch.channels_last))
    per_layer = net._hip_blocks_forward(h.clone(memory_format=torch.channels_last)).permute(0, 2, 3, 1).reshape(x.shape)
    torch.cuda.synchronize()
    for name, g, e in (("cz_tower_c128_bf16 tower output", got, fused["trunk"]), ("cz_tower_heads_c128_bf16 z", z, fused["z"]),
                       ("cz_conv3x3_c128_bf16 layer by layer", per_layer, ref["trunk"])):
        msg = E.describe_mismatch(g, e, "%s, round x 1" % name, E.batch93())
        assert msg is None, msg


@pytest.mark.parametrize("B", [5, 129])
def test_policy_fc_kernel_is_bit_exact(B):
    """cz_fc_heads_f32's policy logits (split-bf16 MFMA, three products) on integer z of up to 16 significant bits (257: hi 256,
    lo 1) and the builder's policy FC (n (1 + c 2^-12): bf16 hi and lo halves, bias with a 2^-12 part): equal to the three-term
    float64 reference; the conditions of exactness are asserted on the reference (exactnets.fc_check)"""
    module = _module("sparse", 1, 0, torch.bfloat16)
    net = _net(module, "bf16")
    z = E.fc_inputs(B)
    fails = E.fc_check(module, z)
    assert not fails, fails
    logits, _ = net._hip_fc_heads(z.cuda().contiguous())
    torch.cuda.synchronize()
    exp = E.fc_reference(module, z)
    got = logits.cpu().double()
    assert not bool(torch.isnan(got).any())
    bad = (got != exp).nonzero()
    assert bad.shape[0] == 0, "cz_fc_heads_f32: %d of %d logits differ; first at row %d, label %d: got %r, expected %r" % (
        bad.shape[0], got.numel(), bad[0, 0], bad[0, 1], float(got[tuple(bad[0])]), float(exp[tuple(bad[0])]))
