"""Exact-arithmetic nets for the trunk kernels (test infrastructure; used by tests/test_exactnets_cpu.py and, on the GPU, by
tests/test_net_exact.py).

If every operand of a conv has few significant bits and every partial sum of an output is an integer multiple of one granule g
and smaller than 2^24 g, an fp32 accumulator holds every partial sum exactly: whatever the MFMA shape, the tiling and the
order of the additions, the kernel must reproduce a float64 evaluation of the same graph BIT FOR BIT.  This module builds such
nets (build), their inputs (planes), the float64 evaluation per engine (reference), the proof obligations under which "bit for
bit" is a theorem (check_exact: conditions on the reference alone), and deliberate corruptions of the reference (MUTATIONS)
with which the suite shows that its inputs would notice a wrong tap, channel, border, position interleave, residual, lo half
or block scale.

Engines: "bf16" / "fp16" (k_tower8_c128), "bf16x2" / "fp16x2" (k_trunk_split_c128), "mx6" (k_trunk_mx_c128), "layer" (the
per-layer bf16 kernels cz_conv3x3_c128_bf16 / cz_tower_c128_bf16 / cz_tower_heads_c128_bf16; cz_conv3x3_c128_bf16 rounds to
bf16 before the residual add, so check_exact also wants the pre-residual sums bf16-exact for this engine).
What the reference models beyond the plain graph: the strict engines' three-term product a_hi w_hi + a_hi w_lo + a_lo w_hi on
halves taken as cchess_zero_amd.net._pack / xs_split4 take them, their clamp of fp16 activations at 65504, mx6 through
tests/mxemu.py in float64, and the split-bf16 three-term product of the policy FC (cz_fc_heads_f32).
In every family but the round ones whatever a kernel stores between layers is already representable in its storage format
(condition (a)): its rounding and quantising code is the identity there.  The round families (ROUND_FAMILIES) put every
activation off that grid; for them the reference applies each engine's storage step explicitly (_store, mxemu's quantiser),
condition (b) is proved element by element, reference(tally=) counts which rounding, saturation and scale cases the step met
(round_cases), and MUTATIONS holds corruptions of the step itself."""
import math

import numpy as np
import torch
import torch.nn.functional as F

import mxemu
from cchess_zero_amd.net import BN_EPS, FILTERS, PROB_SIZE

F64 = torch.float64
BF16, FP16 = torch.bfloat16, torch.float16
ENGINES = ("bf16", "fp16", "bf16x2", "fp16x2", "mx6", "layer")
HALF = {"bf16": BF16, "fp16": FP16, "bf16x2": BF16, "fp16x2": FP16, "mx6": FP16, "layer": BF16}
FAMILIES = ("sparse", "dense", "lo", "lo_subnormal", "mx_cross", "round", "round_x2", "round_mx")
# round: activations deliberately OFF every engine's storage grid (biases with fractional bits, weights with lo halves): the
# reference applies the engine's storage step (_store / the mx6 quantiser) explicitly and tallies which rounding cases it met.
# One net per kind of engine: plain 16-bit stores, hi + lo pairs, mx6
ROUND_FAMILIES = ("round", "round_x2", "round_mx")
ROUND_FAMILY = {"bf16": "round", "fp16": "round", "bf16x2": "round_x2", "fp16x2": "round_x2", "mx6": "round_mx"}
# fractional bits of the round family's biases below the channel's unit S: enough to leave the engine's storage grid (8 / 11
# bits, a pair of them, 11 + 4 for mx6) and few enough for condition (b) with sums of a few dozen S
ROUND_F = {("round", BF16): 10, ("round", FP16): 13, ("round_x2", BF16): 17, ("round_x2", FP16): 17, ("round_mx", FP16): 15}
# lo family: w = n (1 + 2^-k), hi = n and lo = n 2^-k both non-zero NORMAL numbers of the operand type.  A value that went
# through s such layers is M (1 + ~s 2^-k); its hi half stays the integer M (and the granule of the next layer's products
# 2^-k) only while s 2^-k <= 2^-12 (fp16, 11 bits) / 2^-9 (bf16, 8 bits): k = 12 / 9 in EVERY layer would round hi up from
# the second layer on, the products' granule would drop to 2^-21 and condition (b) could not hold for values above 8.  So
# k grows with the number of layers that carry a lo half: (k of the first conv or None, k of the tower layers) by layer count
LO_K = {FP16: {2: (13, 14), 4: (None, 14)}, BF16: {2: (12, 12), 4: (None, 12)}}
DENSE_SEEDS = 3                  # the complementary masks of the dense family: every tower weight entry is non-zero in one of them
DENSE_BIAS = (14.0, 0.0)          # -(this + {0, 1, 2}): first / second conv of the dense family's block
SALT = 2                         # of the builders' random streams: chosen so that check_exact's liveness holds at every depth in use
GROUP = {"bf16": 4, "fp16": 4, "bf16x2": 2, "fp16x2": 2, "mx6": 2, "layer": 1}    # positions per workgroup


# ---------------------------------------------------------------------------------------------------------------------
# builders
def bn_var(scale, device):
    """float32 moving_var with rsqrt(var + BN_EPS) == scale (powers of two) EXACTLY under `device`'s rsqrt; the neighbouring
    floats of float32(1 / scale^2) - float32(1e-5) are searched, those whose sum with BN_EPS is the exact power of four first
    (then the NumPy restatement's 1 / sqrt agrees too)."""
    scale = scale.to(device=device, dtype=torch.float32)
    inv2 = 1.0 / (scale * scale)
    base = (inv2 - BN_EPS).view(torch.int32)
    best = torch.zeros_like(scale)
    found = torch.zeros_like(scale, dtype=torch.bool)
    for want_sum in (True, False):
        for k in (0, 1, -1, 2, -2, 3, -3, 4, -4):
            cand = (base + k).view(torch.float32)
            ok = torch.rsqrt(cand + BN_EPS) == scale
            if want_sum:
                ok &= (cand + BN_EPS) == inv2
            take = ok & ~found
            best = torch.where(take, cand, best)
            found |= take
    assert bool(found.all()), "no float32 moving_var folds to an exact power of two on %s" % device
    return best


def _set_convbn(cb, w, b, rng, mu0=False):
    """make cb.folded() return exactly (w, b): per-channel BN scale 2^j, non-zero moving_mean, conv bias to match (mu0: a zero
    moving_mean, for biases of 24 significant bits, which b + mu would round)"""
    dev = cb.conv.weight.device
    n = w.shape[0]
    s = torch.tensor(2.0 ** rng.integers(-1, 3, n), dtype=torch.float32)          # rsqrt(var + eps) in {1/2, 1, 2, 4}
    mu = torch.tensor(rng.integers(-1, 2, n).astype(np.float32))
    if mu0:
        mu = torch.zeros_like(mu)
    w, b = torch.as_tensor(w, dtype=torch.float32), torch.as_tensor(b, dtype=torch.float32)
    with torch.no_grad():
        cb.moving_var.copy_(bn_var(s, dev))
        cb.moving_mean.copy_((mu / s).to(dev))
        cb.conv.weight.copy_((w / s.view(-1, 1, 1, 1)).to(dev))
        cb.conv.bias.copy_(((b + mu) / s).to(dev))
    fw, fb = cb.folded()
    assert torch.equal(fw.cpu(), w) and torch.equal(fb.cpu(), b), "BN does not fold exactly"


def _sparse_conv(rng, cin, nnz, values, cover_first):
    """[128][cin][3][3] with `nnz` non-zeros per output channel drawn from `values`; the first one of channel o sits at
    (input channel perm[o], tap o % 9) (cover_first) so that every tap and every input channel is used in every layer"""
    w = np.zeros((FILTERS, cin, 3, 3), np.float32)
    perm = rng.permutation(FILTERS) % cin
    for o in range(FILTERS):
        for j in range(nnz[o]):
            while True:
                ci, t = (int(perm[o]), o % 9) if (j == 0 and cover_first) else (int(rng.integers(cin)), int(rng.integers(9)))
                if w[o, ci, t // 3, t % 3] == 0:
                    break
            val = values[rng.integers(len(values))]
            w[o, ci, t // 3, t % 3] = abs(val) if (j == 0 and cover_first) else val      # one positive weight: the channel can fire
    return w


def _sparse_layer(rng, l, scale=1.0):
    """3-4 non-zeros per output channel from {+-1, +-2}, small integer biases.  The first conv of a block mixes signs (mostly
    +-1); the second one subtracts ({-1, -2}) except for one +1 per channel, so that the residual stream neither dies nor
    outgrows 8 significant bits (what the bf16 engine stores) within 7 blocks"""
    odd = l & 1
    values = [-1.0, -1.0, -2.0] if odd else [1.0, -1.0] * 15 + [2.0, -2.0]
    w = _sparse_conv(rng, FILTERS, rng.integers(3, 5, FILTERS), values, True)
    if odd:
        w[w > 0] = 1.0
    b = rng.choice([0.0, 0.0, 1.0] if odd else [0.0, 0.0, 0.0, 0.0, 1.0], FILTERS).astype(np.float32)
    return w * scale, b * scale


def _positive_layer(rng, scale):
    """2-3 non-zeros per output channel from {1, 1, 1, 2}, no bias: nothing cancels, so a value M (1 + c 2^-k) keeps the integer
    M as its hi half and c M 2^-k as its lo half through every layer (a difference of two such values with different c would
    leave a hi half of a few 2^-k, and the next layer's a_hi w_lo products a granule of 2^-2k)"""
    w = _sparse_conv(rng, FILTERS, rng.integers(2, 4, FILTERS), [1.0, 1.0, 1.0, 2.0], True)
    return w * scale, np.zeros(FILTERS, np.float32)


def _first_conv_sparse(rng, scale=1.0):
    """a few +-1 per output channel; channel o < 126 has +1 at (plane o // 9, tap o % 9): every neighbour of an impulse lights up"""
    w = _sparse_conv(rng, 14, np.full(FILTERS, 3), [1.0, -1.0], False)
    for o in range(126):
        w[o, o // 9, (o % 9) // 3, o % 3] = 1.0
    b = np.where(np.arange(FILTERS) < 126, 0.0, 1.0).astype(np.float32)                  # two channels with a bias: always on
    return w * scale, b * scale


# round family: the 16 channels {32 t + 8 q + 4 h + i} that share an mx6 activation scale form one class (kind, log2 of its unit
# S; the tiny class's unit depends on the half type).  A tower layer has ONE weight per output channel, from a channel of the
# same class: no sum mixes magnitudes, and condition (b) holds element by element over 2^-120 .. 2^17
_ROUND_CLASSES = (("ord", 0), ("ord", 4), ("lone_p", 8), ("lone_u", -4), ("ord", -9), ("tiny", None), ("huge", 0), ("sparse", 1))
_ROUND_HUGE = (-2000.0, -600.0, -250.0, 4.0, 9.0, 4.0, 9.0, 30.0, 500.0)      # first conv bias - 65504 of the huge class


def _frac(rng, F, n):
    """n values in [0, 1) on the 2^-F grid whose trailing bits are 0 .. 0 or 1 0 .. 0 at a random depth: exact values, values just
    above and below a storage grid point, and ties at every depth"""
    j = rng.integers(0, 2 ** F, n)
    t = rng.integers(0, F + 1, n)
    j = (j >> t) << t
    j = j | np.where((rng.random(n) < 0.5) & (t > 0), 1 << np.maximum(t - 1, 0), 0)
    return j * 2.0 ** -F


def _round_net(rng, nl, family, half):
    """-> (w0, b0, [(w, b)] tower, (head w [3,128], head b [3]), lo layers).  Channel c has a unit u_c = S 2^-j of its class;
    first conv: u_c (k + n + f), k the number of its three (plane, tap) entries that are hit, n a small integer, f a fraction of
    ROUND_F bits (_frac); tower layer: b + w a[p] (+ x), p a channel of the same class, w = n u_c / u_p: every term is a multiple of
    u_c 2^-F.  Constant channels (no weights) pin the cases no random draw meets: the tie at half the smallest fp16 subnormal,
    an mx6 group maximum that is a power of two / rounds up to one, the E2M3 tie at 1/16.  Engines with lo halves: in the first
    conv of a block every fourth channel has w (1 + 2^-k) and no bias"""
    F = ROUND_F[(family, half)]
    lo_k = None if family == "round" else 12 if half == FP16 else 9
    mx = family == "round_mx"
    Fh = min(4, F - 10)
    classes = list(_ROUND_CLASSES)
    if lo_k is not None:
        # the class with lo halves: values 2 .. 4 of few bits after the first conv, w = 1 + 2^-k in the first conv of a block, no
        # biases in the tower.  A stored pair has 16 / 22 bits RELATIVE to its own size, so it can only be added to terms of
        # its own size: 4 .. 8 after one block, 8 .. 16 after two
        classes[1] = ("lo", 0)
    grp = np.array([2 * (c // 32) + (c % 8) // 4 for c in range(FILTERS)])
    members = [np.nonzero(grp == g)[0] for g in range(8)]
    kind = np.array([classes[g][0] for g in grp])
    tiny_e = -16 if half == FP16 else -120
    expo = np.array([tiny_e if classes[g][1] is None else classes[g][1] for g in grp])
    j = rng.choice([0, 0, 1, 2, 3], FILTERS)
    j = np.where((kind == "lone_p") | (kind == "lone_u"), rng.integers(3, 8, FILTERS), j)
    j = np.where((kind == "huge") | (kind == "lo"), 0, j)
    const = {}                                    # channel -> its value after store s, in units of S (s = 0: the first conv)
    gp, gu, gt = (members[[c[0] for c in classes].index(k)] for k in ("lone_p", "lone_u", "tiny"))
    const[gp[0]] = lambda s: 2.0 ** (1 + s)                               # group maximum: a power of two
    const[gp[1]] = lambda s: 2.0 ** (1 + s) / 64.0                        # 1 / 16 under that group's scale
    const[gp[2]] = lambda s: 2.0 ** (1 + s) * (0.25 + 2.0 ** -17)         # ... and a lo half that is 2^-11 / 16 under it
    const[gu[0]] = lambda s: 2.0 ** (1 + s) * (1.0 - 2.0 ** -13)          # group maximum: rn16 reaches the power of two
    tail = {gt[0]: 1, gt[1]: 1}                                           # bias: -(less than half the smallest subnormal)
    fixed = {gt[2]: 2.0 ** -25} if half == FP16 else {}                   # bias: the tie at half the smallest subnormal
    for c in list(const) + list(tail) + list(fixed):
        j[c] = 0
    unit = 2.0 ** (expo - j).astype(np.float64)
    tail_v = -(2.0 ** -30) if half == FP16 else -(2.0 ** -136)
    delta = rng.choice(_ROUND_HUGE, FILTERS)

    def biases(which, last):
        # (the bf16 tiny class keeps two fractional bits: every value but the tail stays a NORMAL fp32 / bf16 number)
        f = _frac(rng, F, FILTERS)
        if half == BF16:
            f = np.where(kind == "tiny", _frac(rng, 2, FILTERS), f)
        base = {"first": rng.choice([0, 1, 2, -1], FILTERS, p=[0.3, 0.3, 0.3, 0.1]), "conv1": rng.choice([-1, 0, 0, 0, 1], FILTERS),
                "conv2": rng.choice([-3, -2, -1, -1], FILTERS)}[which]
        base = np.where((kind == "lone_p") | (kind == "lone_u"), 0, base)       # (their inputs are 2^-3 .. 2^-7 of the constants)
        if which == "conv2":
            base = np.where(kind == "tiny", 0, base)      # (a negative subnormal kept by relu_before_sign reaches a positive sum)
        b = unit * (base + f)
        sp = kind == "sparse"
        b = np.where(sp, -unit * ((1.0 + f / 2) if which == "first" else (f % 0.25)), b)
        fh = _frac(rng, Fh, FILTERS) if Fh > 0 else np.zeros(FILTERS)
        d = np.where(last & mx, -1000.0 - np.abs(delta), delta)
        b = np.where(kind == "huge", {"first": 65504.0, "conv1": 0.0, "conv2": -65504.0}[which] + d + fh, b)
        # (lo class, split engines: one bit more than hi holds, and that bit set: every hi is a tie, which only a_hi w_lo shows)
        Fl = 6 if mx else 10 if half == FP16 else 7
        fl = _frac(rng, Fl, FILTERS)
        fl = fl if mx else np.floor(fl * 2.0 ** (Fl - 1)) * 2.0 ** (1 - Fl) + 2.0 ** -Fl
        b = np.where(kind == "lo", unit * (2.0 + fl) if which == "first" else 0.0, b)
        for c in tail:
            b[c] = tail_v
        for c, v in fixed.items():
            b[c] = v
        return b

    # first conv: three entries u_c per channel (2 u_c: sparse, 256: huge), none for the constant channels
    w0 = np.zeros((FILTERS, 14, 3, 3))
    b0 = biases("first", False)
    for o in range(FILTERS):
        if o in const:
            b0[o] = const[o](0) * 2.0 ** expo[o]
            continue
        for _ in range(3):
            w0[o, rng.integers(14), rng.integers(3), rng.integers(3)] = unit[o] * {"sparse": 2.0, "huge": 256.0, "lo": 0.25}.get(kind[o], 1.0)
    tower, lo_layers = [], []
    for l in range(nl):
        odd, last = l & 1, l == nl - 1
        w = np.zeros((FILTERS, FILTERS, 3, 3))
        b = biases("conv2" if odd else "conv1", last)
        perm = np.arange(FILTERS)
        for m in members:
            perm[m] = rng.permutation(m)
        n = rng.choice([1.0, 1.0, 1.0, 2.0], FILTERS)
        n = np.where(b < 0, 2.0, n)                 # (a channel with a negative bias can still fire)
        for o in range(FILTERS):
            if o in const:
                b[o] = (const[o](l + 1) - (const[o](l - 1) if odd else 0.0)) * 2.0 ** expo[o]
                continue
            t, p = (o + l) % 9, int(perm[o])
            if kind[o] == "tiny" and odd and o not in tail and o not in fixed:
                t = 4          # the centre tap: a negative subnormal that relu_before_sign keeps (it sits where a tap left the board) is read
            wv = n[o] * unit[o] / unit[p]
            if kind[o] == "huge":
                wv = 1.0
            elif kind[o] == "lo":
                # fp16x2 keeps 23 of the 24 bits of w a: such values add up exactly once (res + t < 8), not twice.  Its second
                # block passes the class through (and mx6, whose cross terms keep 4 bits, has lo halves there as well)
                wv = 1.0 + 2.0 ** -lo_k if not odd and (l == 0 or mx) else 0.0 if (l == 3 and not mx and half == FP16) else 1.0
            w[o, p, t // 3, t % 3] = wv
        if lo_k is not None and not odd and (l == 0 or mx):
            lo_layers.append(l)
        tower.append((w, b))
    # heads: two channels each of one class, in the channels' units (policy 0: + and -, so that cout_swap tells them apart)
    hw = np.zeros((3, FILTERS))
    for h, g in enumerate((0, 1, 4)):
        free = [c for c in members[g] if c not in const and c not in tail and c not in fixed]
        hw[h, free[0]], hw[h, free[1]] = 1.0 / unit[free[0]], (-1.0 if h == 0 else 1.0) / unit[free[1]]
    return w0, b0, tower, (hw, np.array([1.0, 0.0, -1.0])), lo_layers


def build(module, family, seed, half=FP16):
    """Fill `module` (PolicyValueModule, on the device it will be evaluated on) in place: first conv, every tower layer, both
    head convs and policy_fc, so that ConvBN.folded() returns exactly the family's dyadic weights and biases (asserted with
    torch.equal).  half: the operand type of the engine (it selects k of the lo families).  -> module"""
    assert family in FAMILIES
    rng = np.random.default_rng([FAMILIES.index(family), seed, module.res_block_nums, SALT])
    layers = [cb for blk in module.blocks for cb in blk]
    nl = len(layers)
    meta = {"family": family, "seed": seed, "half": half, "lo_layers": []}
    if family == "sparse":
        w0, b0 = _first_conv_sparse(rng)
        tower = []
        for l in range(nl):
            w, b = _sparse_layer(rng, l)
            tower.append((w, b))
    elif family == "dense":
        # first conv: {-1, 0, 1}, a tenth non-zero; tower: +-1 where (entry + layer) % 3 == seed % 3, negative biases that keep
        # the block output inside 8 significant bits (the bf16 engine stores it)
        w0 = (rng.integers(0, 2, (FILTERS, 14, 3, 3)) * 2 - 1) * (rng.random((FILTERS, 14, 3, 3)) < 0.10)
        for o in range(FILTERS):
            w0[o, o % 14, (o % 9) // 3, o % 3] = 1                 # one positive weight: the channel can fire
        b0 = np.zeros(FILTERS, np.float32)
        tower = []
        idx = np.arange(FILTERS * FILTERS * 9).reshape(FILTERS, FILTERS, 3, 3)
        for l in range(nl):
            mask = ((idx + idx // 9 + idx // (9 * FILTERS) + l) % DENSE_SEEDS) == (seed % DENSE_SEEDS)
            w = (rng.integers(0, 2, idx.shape) * 2 - 1) * mask
            b = -(DENSE_BIAS[l % 2] + rng.integers(0, 3, FILTERS))
            tower.append((w.astype(np.float32), b.astype(np.float32)))
    elif family == "lo":
        k0, k = LO_K[half][nl]
        f = 1.0 + 2.0 ** -k
        w0, b0 = _first_conv_sparse(rng, 1.0 if k0 is None else 1.0 + 2.0 ** -k0)
        tower = [_positive_layer(rng, f) for l in range(nl)]
        meta["lo_layers"] = list(range(nl))
    elif family == "lo_subnormal":
        # tower weights n (1/16 + 2^-16), n in {+-1, +-2}: fp16 hi = n / 16, lo = n 2^-16 < 2^-14 is SUBNORMAL in fp16 (as nearly
        # every lo half of a glorot weight is), and so are the lo halves of the activations (K 2^-16, J 2^-19).  (2^-18 would put
        # the products' granule at 2^-22: no room for a residual above 4 under condition (b).)
        assert half == FP16
        w0, b0 = _first_conv_sparse(rng)
        f = 2.0 ** -4 + 2.0 ** -16
        tower = [_positive_layer(rng, f) for l in range(nl)]
        meta["lo_layers"] = list(range(nl))
    elif family in ROUND_FAMILIES:
        assert (family, half) in ROUND_F
        w0, b0, tower, heads, meta["lo_layers"] = _round_net(rng, nl, family, half)
    else:
        # mx_cross: one tower layer (seed % layers) has w = 1 + 2^-12: w_hi = 1 and 2^11 w_lo = 1/2 are E2M3 values under their
        # block's scale (1/4); every other weight is 1.  Activations then are M + L 2^-12 with small integers L <= M < 16 (2^-11
        # would round the fp16 hi half of 3 (1 + 2^-11) up): a_hi = M and 2^11 a_lo = L / 2 sit on the E2M3 grid of their
        # 16-channel group under any scale it can have (check_exact verifies it)
        assert half == FP16
        w0, b0 = _first_conv_sparse(rng)
        lo_layer = seed % nl
        tower = []
        for l in range(nl):
            # all weights 1 and nothing cancels: 2^11 a_lo <= a_hi element by element.  One weight per channel (a shift of one
            # input channel) except in the second conv of the first block (1-2) and in the last layer (4-5, its output is not
            # quantised): the quantised activations stay integers below 16, every one of which is an E2M3 value under any scale
            nnz = rng.integers(4, 6, FILTERS) if l == nl - 1 else rng.integers(1, 3, FILTERS) if l == 1 else np.full(FILTERS, 1)
            w = _sparse_conv(rng, FILTERS, nnz, [1.0], True)
            if l == lo_layer:
                w = w * (1.0 + 2.0 ** -12)
            tower.append((w, np.zeros(FILTERS, np.float32)))
        meta["lo_layers"] = [lo_layer]
    rnd = family in ROUND_FAMILIES
    _set_convbn(module.conv_in, w0, b0, rng, rnd)
    for cb, (w, b) in zip(layers, tower):
        _set_convbn(cb, w, b, rng, rnd)
    # head 1x1 convs: {-1, 0, 1}, a quarter non-zero, small integer biases (fp32 in every engine)
    for cb in (module.policy_conv, module.value_conv):
        n = cb.conv.weight.shape[0]
        if rnd:
            rows = slice(0, 2) if n == 2 else slice(2, 3)
            _set_convbn(cb, heads[0][rows].reshape(n, FILTERS, 1, 1), heads[1][rows], rng, True)
            continue
        w = (rng.integers(0, 2, (n, FILTERS, 1, 1)) * 2 - 1) * (rng.random((n, FILTERS, 1, 1)) < (0.03 if family == "lo_subnormal" else 0.25))
        _set_convbn(cb, w.astype(np.float32), rng.integers(-1, 2, n).astype(np.float32), rng)
    # policy FC: n (1 + c 2^-12), n in {+-1, +-2}, a quarter non-zero: up to 14 significant bits, hi and lo bf16 halves
    w = rng.choice([1.0, -1.0, 2.0, -2.0], (PROB_SIZE, 180)) * (rng.random((PROB_SIZE, 180)) < 0.25)
    w = w * (1.0 + rng.integers(0, 2, w.shape) * 2.0 ** -12)
    b = rng.integers(-3, 4, PROB_SIZE) + rng.integers(-2, 3, PROB_SIZE) * 2.0 ** -12
    with torch.no_grad():
        module.policy_fc.weight.copy_(torch.tensor(w, dtype=torch.float32))
        module.policy_fc.bias.copy_(torch.tensor(b, dtype=torch.float32))
    module.exact_meta = meta
    return module


def prefix_module(module, k):
    """a k-block PolicyValueModule on the first k blocks of `module`'s weights (same device): its trunk output is layer 2k"""
    from cchess_zero_amd.net import PolicyValueModule
    m = PolicyValueModule(k).to(module.conv_in.conv.weight.device)
    sd = {n: v for n, v in module.state_dict().items() if not n.startswith("blocks.") or int(n.split(".")[1]) < k}
    m.load_state_dict(sd)
    m.exact_meta = dict(module.exact_meta, lo_layers=[l for l in module.exact_meta["lo_layers"] if l < 2 * k])
    return m


# ---------------------------------------------------------------------------------------------------------------------
# inputs
def planes(kind, n=None, group=2, seed=0):
    """0/1 planes [B,9,10,14] float32.
    impulses: 90 positions, position i has one single 1, at cell i (y = i // 10, x = i % 10), in plane (5 i) mod 14;
    pairs:    n rows; row r (position r % group of workgroup r // group) carries impulse (7 r) mod 90 when position + workgroup is
              even, the rows between are dense: every impulse has dense workgroup partners (a leak between the positions that
              share a workgroup then shows in the impulse row), at alternating positions from one workgroup to the next;
    dense:    n random positions with about 32 ones each."""
    rng = np.random.default_rng([17, seed])
    if kind == "impulses":
        x = np.zeros((90, 9, 10, 14), np.float32)
        for i in range(90):
            x[i, i // 10, i % 10, (5 * i) % 14] = 1.0
        return torch.from_numpy(x if n is None else x[:n])
    if kind == "dense":        # (rows are drawn one after the other: a shorter batch is a prefix of a longer one)
        return torch.from_numpy((rng.random((3 if n is None else n, 9, 10, 14)) < 32.0 / 1260.0).astype(np.float32))
    assert kind == "pairs"
    n = 2 * group if n is None else n
    x = (rng.random((n, 9, 10, 14)) < 32.0 / 1260.0).astype(np.float32)
    for r in range(n):
        if (r % group + r // group) % 2 == 0:
            i = (7 * r) % 90
            x[r] = 0.0
            x[r, i // 10, i % 10, (5 * i) % 14] = 1.0
    return torch.from_numpy(x)


def impulse_cells(x):
    """[B] int: the cell of a row's single 1, or -1 for a row that is no impulse"""
    flat = x.reshape(x.shape[0], 90, -1).sum(-1)
    one = (flat.sum(1) == 1)
    return torch.where(one, flat.argmax(1), torch.full_like(flat.argmax(1), -1))


# ---------------------------------------------------------------------------------------------------------------------
# float64 references
def _halves(t, hdt):
    """t: float64 holding fp32 values -> (hi, lo) as net._pack / xs_split4 take them: hi = rn16(t), lo = rn16(t - hi)"""
    t32 = t.float()
    hi = t32.to(hdt)
    lo = (t32 - hi.float()).to(hdt)
    return hi.double(), lo.double()


def _conv(a, w, wrap=False):
    """3x3 SAME conv in float64; wrap: the off-board tap of cell (y, 9) reads cell (y + 1, 0) — the neighbouring LDS row of a
    kernel that forgets the border mask"""
    ap = F.pad(a, (1, 1, 1, 1))
    if wrap:
        ap[:, :, 1:9, 11] = a[:, :, 1:9, 0]
    return F.conv2d(ap, w)


def _granule(t):
    """largest power of two of which every entry of t is an integer multiple (inf for an all-zero tensor)"""
    t = t[t != 0]
    if t.numel() == 0:
        return math.inf
    m, e = torch.frexp(t.abs().double())
    mi = (m * 2.0 ** 53).to(torch.int64)
    low = (mi & -mi).double()
    return 2.0 ** int((e.to(torch.int64) - 53 + torch.log2(low).to(torch.int64)).min())


def _low_log2(t):
    """log2 of the lowest set bit of every entry (the entry's own granule), +inf for a zero"""
    m, e = torch.frexp(t.abs().double())
    mi = (m * 2.0 ** 53).to(torch.int64)
    low = (mi & -mi).clamp(min=1).double()
    return torch.where(t == 0, math.inf, (e - 53).double() + torch.log2(low))


# ---------------------------------------------------------------------------------------------------------------------
# the storage step of every engine, in float64 on values that are exact fp32 numbers
_FMT = {FP16: (-14, 11), BF16: (-126, 8)}       # (exponent of the smallest normal, significant bits)


def _ulp(t, hdt):
    """spacing of hdt's values in the binade of |t| (the subnormal spacing below the smallest normal)"""
    emin, p = _FMT[hdt]
    _, e = torch.frexp(t.abs().double())
    return torch.exp2(((e - 1).clamp(min=emin) - (p - 1)).double())


def _round16(t, hdt, mode="rne"):
    """t rounded to hdt: "rne" is the conversion the kernels use (pack_pair; fp16 overflows to inf from 65520 on); "rtz" and
    "half_away" are deliberate corruptions (MUTATIONS)"""
    if mode == "rne":
        return t.float().to(hdt).double()
    u = _ulp(t, hdt)
    q = t / u
    return (torch.trunc(q) if mode == "rtz" else torch.sign(q) * torch.floor(q.abs() + 0.5)) * u


def _store(y, engine, mut=None):
    """What `engine` keeps of a conv output y (bias and residual added, before the ReLU).  -> (v, halves)
    bf16 / fp16 (k_tower8_c128 store_layer): RNE to 16 bits FIRST, then ReLU as a signed 16-bit max with 0 (a negative sum,
        however tiny, and -0 become +0), then, fp16 only, a signed 16-bit min with 0x7BFF: everything from 65520 on (inf) is 65504;
    bf16x2 / fp16x2 (k_trunk_split_c128 xs_split4): clamp to [0, 65504] (bf16: [0, inf)), hi = rn16(v), lo = rn16(v - hi);
        v = hi + lo is what the next layer, the residual (xreg holds the halves), the trunk dump and the heads see: halves = (hi, lo);
    mx6 (k_trunk_mx_c128 store_tile): clamp to [0, 65504]; v stays fp32 (it is the residual); the next conv quantises it.
    mut: a key of MUTATIONS that corrupts this step"""
    hdt = HALF[engine]
    mode = {"store_rtz": "rtz", "store_half_away": "half_away"}.get(mut, "rne")
    top = 65504.0 if hdt == FP16 and mut != "no_top_clamp" else math.inf
    tiny = 2.0 ** _FMT[hdt][0]
    if engine in ("bf16", "fp16"):
        r = _round16(y, hdt, mode)
        v = torch.where(r > 0, r, torch.zeros_like(r))
        if mut == "relu_before_sign":
            v = torch.where((r < 0) & (r > -tiny), r, v)
        return v.clamp(max=top), None
    v = y.clamp(min=0.0, max=top)
    if mut == "relu_before_sign":
        v = torch.where((y < 0) & (y > -tiny), y, v)
    if engine == "mx6":
        return v, None
    hi = _round16(v, hdt, mode)
    lo = _round16(v - hi, hdt, "rtz" if mut == "lo_rtz" else "rne")
    return hi + lo, (hi, lo)


def _count(tally, kind, case, mask):
    if tally is not None:
        tally[(kind, case)] = tally.get((kind, case), 0) + int(mask.sum())


def _tally_round(tally, kind, pre, x, r, hdt):
    """down / up / the two ties / a carry into the next binade, of x -> r = rn16(x)"""
    u = _ulp(x, hdt)
    q = x.abs() / u
    tie = (q - torch.floor(q)) == 0.5
    fin = torch.isfinite(r) & (x != 0)
    _count(tally, kind, pre + "down", fin & ~tie & (r.abs() < x.abs()))
    _count(tally, kind, pre + "up", fin & ~tie & (r.abs() > x.abs()))
    _count(tally, kind, pre + "tie_down", fin & tie & (r.abs() < x.abs()))
    _count(tally, kind, pre + "tie_up", fin & tie & (r.abs() > x.abs()))
    _count(tally, kind, pre + "carry", fin & (r.abs() > x.abs()) & (torch.frexp(r)[1] > torch.frexp(x)[1]))


def _tally_store(tally, kind, engine, y, halves):
    """which cases of the issue's list the storage step of one layer met (counted on the reference alone)"""
    if tally is None:
        return
    hdt = HALF[engine]
    emin, p = _FMT[hdt]
    pos = y > 0
    x = torch.where(pos, y, torch.zeros_like(y))
    if hdt == FP16:
        _count(tally, kind, "over_65504", (y > 65504.0) & (y < 65520.0))
        _count(tally, kind, "over_65520", y >= 65520.0)
        x = torch.where(y >= 65520.0, torch.zeros_like(y), x)
        if engine != "fp16":
            x = x.clamp(max=65504.0)
    r = _round16(x, hdt)
    _tally_round(tally, kind, "", x, r, hdt)
    _count(tally, kind, "neg_tiny", (y < 0) & (y > -(2.0 ** (emin - p))))          # below half the smallest subnormal
    _count(tally, kind, "neg", y <= -(2.0 ** emin))
    if hdt == FP16:
        _count(tally, kind, "subnormal", (r > 0) & (r < 2.0 ** -14))
        _count(tally, kind, "tie_half_min", y == 2.0 ** -25)
    if halves is not None:
        hi, lo = halves
        d = x - hi
        _tally_round(tally, kind, "lo_", d, lo, hdt)
        _count(tally, kind, "lo_neg", lo < 0)
        _count(tally, kind, "lo_zero", (d != 0) & (lo == 0))
        if hdt == FP16:
            _count(tally, kind, "lo_subnormal", (lo != 0) & (lo.abs() < 2.0 ** -14))


def round_cases(engine):
    """the cases of the storage step that the round family must meet for `engine` (keys of reference()'s tally, per layer kind)"""
    c = ["down", "up", "tie_down", "tie_up", "carry", "neg_tiny", "neg"]
    if engine in ("fp16", "fp16x2"):
        c += ["over_65504", "over_65520", "subnormal", "tie_half_min"]
    if engine in ("bf16x2", "fp16x2"):
        c += ["lo_down", "lo_up", "lo_tie_down", "lo_tie_up", "lo_neg", "lo_zero"] + (["lo_subnormal"] if engine == "fp16x2" else [])
    if engine == "mx6":
        c += [p + k for p in ("hi_", "lo_") for k in ("down", "up", "tie_down", "tie_up", "subnormal", "tie_16th")]
        c += ["lo_neg", "g_saturates", "g_hi_reaches_pow2", "g_pow2", "g_zero", "g_65504"]
    return c


ROUND_KINDS = ("first conv", "first conv of a block", "second conv of a block")


def _tally_mx(tally, kind, info, v):
    """the same for the mx6 quantiser of the conv that reads v: info from mxemu.mxq_pair ([cells, 8 groups, 16])"""
    if tally is None:
        return
    for pre, x in (("hi_", info["x0"]), ("lo_", info["x1"])):
        ax = x.abs()
        step = torch.exp2(torch.floor(torch.log2(ax.clamp(min=1.0, max=7.5))) - 3)
        q = ax / step
        tie = ((q - torch.floor(q)) == 0.5) & (ax < 7.5)
        r = mxemu.q_e2m3(x).abs()
        ok = ax <= 7.5
        _count(tally, kind, pre + "down", ok & ~tie & (r < ax))
        _count(tally, kind, pre + "up", ok & ~tie & (r > ax))
        _count(tally, kind, pre + "tie_down", tie & (r < ax))
        _count(tally, kind, pre + "tie_up", tie & (r > ax))
        _count(tally, kind, pre + "subnormal", (ax > 0) & (ax < 1.0))
        _count(tally, kind, pre + "tie_16th", ax == 1.0 / 16)
    _count(tally, kind, "lo_neg", info["x1"] < 0)
    amax, hmax = info["amax"], info["x0"].abs().amax(-1)
    m, _ = torch.frexp(amax)
    _count(tally, kind, "g_saturates", (hmax >= 7.75) & (hmax < 8.0))
    _count(tally, kind, "g_hi_reaches_pow2", hmax == 8.0)
    _count(tally, kind, "g_pow2", (amax > 0) & (m == 0.5))
    _count(tally, kind, "g_zero", amax == 0)
    _count(tally, kind, "g_65504", amax == 65504.0)
    tally.setdefault("bytes", set()).update(info["byte"].unique().tolist())


MUTATIONS = {
    # name: (what the corrupted reference does, needs lo halves, mx6 only)
    "tap_dydx": ("taps (dy, dx) = (-1, 0) and (0, -1) of one layer swapped", False, False),
    "cin_swap": ("two input channels of one layer swapped", False, False),
    "cout_swap": ("two output channels of one layer swapped", False, False),
    "wrap": ("the off-board tap of cell (y, 9) reads cell (y + 1, 0) in one layer", False, False),
    "pos_swap": ("positions i and i ^ 1 exchanged for one layer", False, False),
    "no_residual": ("the residual of one block left out", False, False),
    "lo_zero": ("the lo halves of one tap of one layer zeroed", True, False),
    "scale_off": ("one E2M3 weight block scale off by one", True, True),
    # the storage step of ONE layer corrupted (the output of the first conv of the block whose second conv the others corrupt);
    # round families only: everywhere else that step is the identity
    "store_rtz": ("a layer's 16-bit store (the hi half) truncates instead of rounding to nearest even", False, False),
    "store_half_away": ("a layer's 16-bit store (the hi half) rounds ties away from zero", False, False),
    "no_top_clamp": ("a layer's fp16 store does not saturate at 65504", False, False),
    "relu_before_sign": ("a layer's store keeps a negative sum that is subnormal (or -0) in fp16 instead of storing +0", False, False),
    "lo_rtz": ("a layer's lo half truncates", False, False),
    "q6_rtz": ("the E2M3 conversion of a layer's activations truncates", False, True),
    "q6_half_away": ("the E2M3 conversion of a layer's activations rounds ties away from zero", False, True),
    "q6_no_sat": ("the E2M3 conversion of a layer's activations rounds [7.75, 8] to 8 instead of saturating at 7.5", False, True),
    "scale_from_hi": ("a layer's activation block scale is taken from hi = rn16(v) instead of v", False, True),
}
# Not in the list: "scale_no_clamp" (the scale byte of an all-zero group not clamped at 1).  No output can see it: every operand
# of such a group is zero under any scale.  relu_before_sign is confined to the engines with fp16 halves: a bf16 has fp32's
# exponent range, so a negative sum that rounds to -0 or to a bf16 subnormal is an fp32 subnormal, which this family keeps to
# one bias (-2^-136) and never multiplies.
_STORE_MUTATIONS = {"store_rtz": ENGINES[:5], "store_half_away": ENGINES[:5],
                    "no_top_clamp": ("fp16", "fp16x2"), "relu_before_sign": ("fp16", "fp16x2", "mx6"), "lo_rtz": ("bf16x2", "fp16x2"),
                    "q6_rtz": ("mx6",), "q6_half_away": ("mx6",), "q6_no_sat": ("mx6",), "scale_from_hi": ("mx6",)}


def applicable_mutations(family, engine, B):
    out = []
    for name, (_, needs_lo, mx_only) in MUTATIONS.items():
        if name in _STORE_MUTATIONS and (family not in ROUND_FAMILIES or engine not in _STORE_MUTATIONS[name]):
            continue
        if needs_lo and (family in ("sparse", "dense", "round") or engine not in ("bf16x2", "fp16x2", "mx6")):
            continue
        if mx_only and engine != "mx6":
            continue
        if name == "pos_swap" and B < 2:
            continue
        out.append(name)
    return out


class _Checks:
    """collects check_exact's conditions while the reference is evaluated"""

    def __init__(self, engine):
        self.engine, self.fail, self.max_ratio, self.max_act = engine, [], 0.0, 0.0

    def weights(self, name, w, hi=None, lo=None):
        hdt = HALF[self.engine]
        if hi is None:
            if not torch.equal(w.float().to(hdt).double(), w):
                self.fail.append("%s: weights are not exact in %s" % (name, hdt))
        elif not torch.equal(hi + lo, w):
            self.fail.append("%s: weights are not exact as a hi + lo pair" % name)

    def accumulation(self, name, terms, bias, res):
        """(b): sum |a| |w| + |bias| + |residual| < 2^24 g with g the common granule of products, bias and residual"""
        g = min([_granule(a) * _granule(w) for a, w in terms if a.numel() and _granule(a) < math.inf and _granule(w) < math.inf]
                + [_granule(bias)] + ([_granule(res)] if res is not None else []))
        if g == math.inf:
            return
        tot = sum(F.conv2d(F.pad(a.abs(), (1, 1, 1, 1)), w.abs()) for a, w in terms) + bias.abs().view(1, -1, 1, 1)
        if res is not None:
            tot = tot + res.abs()
        r = float(tot.max()) / (2.0 ** 24 * g)
        self.max_ratio = max(self.max_ratio, r)
        if not r < 1.0:
            self.fail.append("%s: sum |a w| + |b| + |res| = %.6g is not below 2^24 granules of %.3g" % (name, float(tot.max()), g))

    def stored(self, name, v, pre=None):
        """(a): v survives the engine's storage format"""
        e, hdt = self.engine, HALF[self.engine]
        self.max_act = max(self.max_act, float(v.abs().max()))
        if e in ("bf16", "fp16", "layer"):
            ok = torch.equal(v.float().to(hdt).double(), v)
            if e == "layer" and pre is not None:
                ok = ok and torch.equal(pre.float().to(hdt).double(), pre)
        elif e == "mx6":
            ok = torch.equal(v.float().double(), v)
        else:
            hi, lo = _halves(v, hdt)
            ok = torch.equal(v.float().double(), v) and torch.equal(hi + lo, v)
        if not ok:
            self.fail.append("%s: a stored value does not survive the storage format of %s (largest %.6g)" % (name, e, float(v.abs().max())))

    def accumulation_each(self, name, terms, bias, res, pad=1):
        """(b) element by element (round families, whose channels span 2^-120 .. 2^17): for EVERY output element
        sum |a| |w| + |bias| + |residual| < 2^24 g, g the granule of that element's own products, bias and residual"""
        L = None
        for a, w in terms:
            La, Lw = F.pad(_low_log2(a), (pad,) * 4, value=math.inf), _low_log2(w)
            if L is None:
                L = torch.full((a.shape[0], w.shape[0]) + tuple(a.shape[2:]), math.inf, dtype=F64)
            H, W = a.shape[2:]
            for o, c, ky, kx in (w != 0).nonzero().tolist():
                L[:, o] = torch.minimum(L[:, o], La[:, c, ky:ky + H, kx:kx + W] + Lw[o, c, ky, kx])
        L = torch.minimum(L, _low_log2(bias).view(1, -1, 1, 1))
        tot = sum(F.conv2d(F.pad(a.abs(), (pad,) * 4), w.abs()) for a, w in terms) + bias.abs().view(1, -1, 1, 1)
        if res is not None:
            L, tot = torch.minimum(L, _low_log2(res)), tot + res.abs()
        live = torch.isfinite(L)
        if not bool(live.any()):
            return
        r = tot[live] / torch.exp2(L[live] + 24.0)
        self.max_ratio = max(self.max_ratio, float(r.max()))
        if not bool((r < 1.0).all()):
            self.fail.append("%s: %d outputs have sum |a w| + |b| + |res| not below 2^24 of their own granules (worst %.3g)" % (
                name, int((r >= 1.0).sum()), float(r.max())))

    def stored_round(self, name, y, v, fp32_out):
        """(a) of the round families: the value handed to the storage step is a finite exact fp32 number (the stored value is the
        storage step's result by construction); a hi + lo pair is one too (the kernel adds the halves in fp32: residual, trunk
        dump, heads); mx6's last layer is written as fp32 with a ReLU alone, so it stays below the clamp the reference applies"""
        self.max_act = max(self.max_act, float(v.abs().max()))
        if not (bool(torch.isfinite(y).all()) and torch.equal(y.float().double(), y) and torch.equal(v.float().double(), v)):
            self.fail.append("%s: a value handed to the storage step, or a stored hi + lo, is no fp32 number" % name)
        if fp32_out and not float(y.max()) < 65504.0:
            self.fail.append("%s: the fp32 output reaches 65504" % name)

    def on_grid(self, name, pairs):
        for what, q, x in pairs:
            if not torch.equal(q, x):
                self.fail.append("%s: %s is not on the E2M3 grid of its block (%d values)" % (name, what, int((q != x).sum())))


def _tower(module, v, engine, mutation, chk, out, mut_layer=None, halves=None, tally=None, storage=None):
    """the residual tower, the head convs and the policy FC on first-layer activations v [B,128,9,10] float64 (halves: their
    hi + lo pair as a split engine stored them).  Round families: every layer's output goes through the engine's storage step
    (_store), tally counts the cases it met.  storage: "explicit" / "identity" force the step on / off (identity: the clamp alone,
    which is what the step provably is for every other family: condition (a))"""
    hdt = HALF[engine]
    split, mx = engine in ("bf16x2", "fp16x2"), engine == "mx6"
    top = 65504.0 if hdt == FP16 else float("inf")
    meta = getattr(module, "exact_meta", {"lo_layers": []})
    layers = [cb for blk in module.blocks for cb in blk]
    ml = 1 if mut_layer is None else mut_layer                # the layer most mutations corrupt (odd: the second conv of a block)
    assert ml & 1 and ml < len(layers)
    ml_lo = meta["lo_layers"][-1] if meta["lo_layers"] else ml  # ... and the one whose lo halves / block scale are corrupted
    rnd = meta.get("family") in ROUND_FAMILIES
    explicit = engine != "layer" and (rnd if storage is None else storage == "explicit")
    smut = mutation if mutation in _STORE_MUTATIONS else None       # corrupts the store of layer ml - 1 = what layer ml reads
    ms = ml - 1
    if split and smut in ("store_rtz", "store_half_away"):
        # a split engine's lo half makes up for whatever its hi half does: only a_hi w_lo sees hi alone, so these two corrupt what
        # the last layer with lo halves in its weights reads (-1: the first conv's output, _evaluate)
        ms = ml_lo - 1
    kinds = ("second conv of a block", "first conv of a block")       # of the layer whose stored output layer l reads (l >= 1)
    B = v.shape[0]
    err = torch.zeros_like(v) if split else None              # bound on |plain graph - three-term graph|, propagated
    x_in = x_err = None
    for l, cb in enumerate(layers):
        w, b = (t.detach().cpu().double() for t in cb.folded())
        a = v
        if l == ml:
            if mutation == "tap_dydx":
                w = w.clone(); w[:, :, 0, 1], w[:, :, 1, 0] = w[:, :, 1, 0].clone(), w[:, :, 0, 1].clone()
            elif mutation == "cin_swap":
                w = w.clone(); w[:, [3, 100]] = w[:, [100, 3]]
            elif mutation == "cout_swap":
                hw = module.policy_conv.folded()[0][0, :, 0, 0].cpu()          # two channels the policy head tells apart
                c = [int((hw > 0).nonzero()[0]), int((hw < 0).nonzero()[0])]
                w = w.clone(); b = b.clone(); w[c] = w[c[::-1]]; b[c] = b[c[::-1]]
            elif mutation == "pos_swap":
                perm = torch.arange(B) ^ 1
                perm[perm >= B] = B - 1
                a = a[perm]
                halves = None if halves is None else (halves[0][perm], halves[1][perm])
        wrap = mutation == "wrap" and l == ml
        if not (l & 1):
            x_in, x_err = v, err
        res = x_in if (l & 1) and not (mutation == "no_residual" and l == ml) else None
        name = "tower layer %d" % l
        if mx:
            a_hi, a_lo = mxemu.split16(a, F64)
            q6, info, here = mxemu.q_e2m3, ({} if tally is not None else None), l == ml and smut is not None
            if here and smut in ("store_rtz", "store_half_away"):
                a_hi = _round16(a, FP16, smut[6:])
                a_lo = a - a_hi
            elif here and smut.startswith("q6_"):
                q6 = {"q6_rtz": lambda t: mxemu.q_e2m3(t, "rtz"), "q6_half_away": lambda t: mxemu.q_e2m3(t, "half_away"),
                      "q6_no_sat": lambda t: mxemu.q_e2m3(t, sat=False)}[smut]
            w_hi, w_lo = mxemu.split16(w, F64)
            w_lo = w_lo.to(FP16).double()
            if mutation == "lo_zero" and l == ml_lo:
                w_lo[:, :, 2, 0] = 0.0
            a_h6, a_l6 = mxemu.mxq_pair(a_hi, a_lo * mxemu.S_LO, 1, scale_from=a_hi if here and smut == "scale_from_hi" else a,
                                        q=q6, info=info)
            if rnd:
                _tally_mx(tally, "first conv" if l == 0 else kinds[l & 1], info, a)
            w_l6, w_h6 = mxemu.mxq_pair(w_lo * mxemu.S_LO, w_hi, 1)
            if mutation == "scale_off" and l == ml_lo:
                # an output channel whose change reaches the policy head: one the head reads (second conv of a block: the residual
                # stream carries it to the trunk), or one that the next layer feeds into such a channel (first conv of a block)
                co = int((module.policy_conv.folded()[0][0, :, 0, 0].cpu() > 0).nonzero()[0])
                if not (l & 1):
                    co = int((layers[l + 1].folded()[0][co].cpu() != 0).any(-1).any(-1).nonzero()[0])
                ci, ty, tx = (w_hi[co] != 0).nonzero()[0].tolist()                             # the block of its first non-zero weight
                groups = mxemu.group_perm().reshape(8, 16)
                grp = groups[(groups == ci).any(1)][0]
                w_l6, w_h6 = w_l6.clone(), w_h6.clone()
                for t in (w_l6, w_h6):
                    t[co, grp, ty, tx] *= 2.0
            terms = [(a_hi, w_hi), (a_h6, w_l6 / mxemu.S_LO), (a_l6, w_h6 / mxemu.S_LO)]
            if chk is not None:
                chk.weights(name, w, w_hi, w_lo)
                if meta.get("family") == "mx_cross":
                    chk.on_grid(name, [("a_hi", a_h6, a_hi), ("2^11 a_lo", a_l6, a_lo * mxemu.S_LO), ("w_hi", w_h6, w_hi),
                                       ("2^11 w_lo", w_l6, w_lo * mxemu.S_LO)])
        elif split:
            a_hi, a_lo = _halves(a, hdt) if halves is None else halves
            w_hi, w_lo = _halves(w, hdt)
            if chk is not None:
                chk.weights(name, w, w_hi, w_lo)
            dropped = _conv(a_lo.abs(), w_lo.abs()) + _conv(a.abs(), (w - w_hi - w_lo).abs())
            if mutation == "lo_zero" and l == ml_lo:
                w_lo = w_lo.clone(); w_lo[:, :, 2, 0] = 0.0
            terms = [(a_hi, w_hi), (a_hi, w_lo), (a_lo, w_hi)]
            err = _conv(err, w.abs()) + dropped + (x_err if res is not None else 0.0)
        else:
            terms = [(a, w)]
            if chk is not None:
                chk.weights(name, w)
        pre = sum(_conv(ta, tw, wrap) for ta, tw in terms) + b.view(1, -1, 1, 1)
        # "layer" on a round net: cz_conv3x3_c128_bf16 block by block rounds the pre-residual sum to bf16, adds the residual (both
        # bf16, in fp32: asserted exact), applies the ReLU and rounds again
        layer_rnd = engine == "layer" and rnd and storage != "identity"
        y = (_round16(pre, BF16) if layer_rnd else pre) + res if res is not None else pre
        if chk is not None:
            (chk.accumulation_each if rnd else chk.accumulation)(name, terms, b, None if layer_rnd else res)
            if layer_rnd:
                chk.stored_round(name, pre, pre, False)
        fp32_out = mx and l == len(layers) - 1            # store_tile_f32: a ReLU, no storage step
        if explicit and not fp32_out:
            v, halves = _store(y, engine, smut if l == ms else None)
            if rnd:
                _tally_store(tally, kinds[1 - (l & 1)], engine, y, halves)
        else:
            v, halves = y.clamp(min=0.0, max=top), None
            if layer_rnd:
                v = _round16(v, BF16)
        if chk is not None:
            chk.stored_round(name, y, v, fp32_out) if rnd else chk.stored(name, v, pre)
        out["layers"].append(v)
        if split:
            out["bound"].append(err)
    out["trunk"] = v.permute(0, 2, 3, 1).reshape(B, 90, FILTERS)
    if split:
        out["trunk_bound"] = err.permute(0, 2, 3, 1).reshape(B, 90, FILTERS)
    # head 1x1 convs: fp32 weights on the stored trunk values, ReLU
    wp, bp = (t.detach().cpu().double() for t in module.policy_conv.folded())
    wv, bv = (t.detach().cpu().double() for t in module.value_conv.folded())
    hw, hb = torch.cat([wp, wv], 0), torch.cat([bp, bv], 0)
    if chk is not None and rnd:
        chk.accumulation_each("head convs", [(v, hw)], hb, None, pad=0)
    elif chk is not None:
        g = min(_granule(v) * _granule(hw), _granule(hb))
        tot = F.conv2d(v.abs(), hw.abs()) + hb.abs().view(1, -1, 1, 1)
        if g < math.inf and not float(tot.max()) < 2.0 ** 24 * g:
            chk.fail.append("head convs: sum |a w| + |b| = %.6g is not below 2^24 granules of %.3g" % (float(tot.max()), g))
    z = torch.relu(F.conv2d(v, hw, hb)).permute(0, 2, 3, 1).reshape(B, 90, 3)
    out["z"] = z
    out["logits"] = fc_reference(module, z)
    return out


def fc_reference(module, z):
    """policy logits as cz_fc_heads_f32 computes them: z and the weight as bf16 hi + lo, z_hi w_hi + z_hi w_lo + z_lo w_hi + b,
    in float64.  z [B,90,3] (only the two policy channels are read)"""
    p = z[:, :, :2].reshape(z.shape[0], 180).double()
    p_hi, p_lo = _halves(p, BF16)
    w_hi, w_lo = _halves(module.policy_fc.weight.detach().cpu().double(), BF16)
    return p_hi @ w_hi.t() + p_hi @ w_lo.t() + p_lo @ w_hi.t() + module.policy_fc.bias.detach().cpu().double()


def fc_check(module, z):
    """the conditions under which cz_fc_heads_f32's logits equal fc_reference bit for bit; -> list of failures"""
    p = z[:, :, :2].reshape(z.shape[0], 180).double()
    w = module.policy_fc.weight.detach().cpu().double()
    b = module.policy_fc.bias.detach().cpu().double()
    p_hi, p_lo = _halves(p, BF16)
    w_hi, w_lo = _halves(w, BF16)
    fail = []
    if not torch.equal(p_hi + p_lo, p) or not torch.equal(w_hi + w_lo, w):
        fail.append("policy FC: z or the weight is not an exact bf16 hi + lo pair")
    g = min([_granule(a) * _granule(c) for a, c in ((p_hi, w_hi), (p_hi, w_lo), (p_lo, w_hi)) if _granule(a) < math.inf] + [_granule(b)])
    tot = p_hi.abs() @ (w_hi.abs() + w_lo.abs()).t() + p_lo.abs() @ w_hi.abs().t() + b.abs()
    if not float(tot.max()) < 2.0 ** 24 * g:
        fail.append("policy FC: sum |z w| + |b| = %.6g is not below 2^24 granules of %.3g" % (float(tot.max()), g))
    return fail


def _evaluate(module, x, engine, mutation=None, chk=None, mut_layer=None, tally=None, storage=None):
    assert engine in ENGINES and (mutation is None or mutation in MUTATIONS) and storage in (None, "identity", "explicit")
    rnd = getattr(module, "exact_meta", {}).get("family") in ROUND_FAMILIES
    hdt = HALF[engine]
    xn = torch.as_tensor(x).detach().cpu().double().permute(0, 3, 1, 2).contiguous()
    w, b = (t.detach().cpu().double() for t in module.conv_in.folded())
    out = {"layers": [], "bound": []}
    if engine in ("bf16x2", "fp16x2", "mx6"):
        w_hi, w_lo = _halves(w, hdt)                          # the planes are 0/1: only the weights are split
        terms = [(xn, w_hi), (xn, w_lo)]
        if chk is not None:
            chk.weights("first conv", w, w_hi, w_lo)
    else:
        terms = [(xn, w)]
        if chk is not None:
            chk.weights("first conv", w)
    pre = sum(_conv(a, tw) for a, tw in terms) + b.view(1, -1, 1, 1)
    if engine != "layer" and (rnd if storage is None else storage == "explicit"):
        lo_layers = getattr(module, "exact_meta", {}).get("lo_layers", [])
        first = mutation in ("store_rtz", "store_half_away") and engine in ("bf16x2", "fp16x2") and lo_layers and lo_layers[-1] == 0
        v, halves = _store(pre, engine, mutation if first else None)
        if rnd:
            _tally_store(tally, "first conv", engine, pre, halves)
    else:
        v, halves = pre.clamp(min=0.0, max=65504.0 if hdt == FP16 else float("inf")), None
    if chk is not None:
        (chk.accumulation_each if rnd else chk.accumulation)("first conv", terms, b, None)
        chk.stored_round("first conv", pre, v, False) if rnd else chk.stored("first conv", v, pre)
    out["layers"].append(v)
    if engine in ("bf16x2", "fp16x2"):
        out["bound"].append(_conv(xn, (w - w_hi - w_lo).abs()))
    return _tower(module, v, engine, mutation, chk, out, mut_layer, halves, tally, storage)


def reference(module, x, engine, mutation=None, mut_layer=None, tally=None, storage=None):
    """float64 evaluation of the graph as `engine` computes it.  x: planes [B,9,10,14].  -> dict: layers (post-ReLU
    activations [B,128,9,10] after every conv layer, first conv first), trunk [B,90,128], z [B,90,3] (post-ReLU head conv
    outputs), logits [B,2086]; strict engines also bound / trunk_bound: an upper bound on |plain float64 graph - this| from
    the dropped a_lo w_lo products, propagated through the layers.  mutation: a key of MUTATIONS (a corrupted reference);
    mut_layer: the (odd) tower layer it corrupts, default 1 (lo_zero and scale_off corrupt the last layer that carries w_lo)."""
    with torch.no_grad():
        return _evaluate(module, x, engine, mutation, mut_layer=mut_layer, tally=tally, storage=storage)


def tower_reference(module, act, engine="layer", check=False):
    """the same for activations [B,90,128] fed directly to the tower (the per-layer and tower-only kernels); check: assert
    check_exact's conditions (a) and (b) on the way"""
    chk = _Checks(engine) if check else None
    with torch.no_grad():
        v = torch.as_tensor(act).detach().cpu().double().reshape(act.shape[0], 9, 10, FILTERS).permute(0, 3, 1, 2).contiguous()
        out = _tower(module, v, engine, None, chk, {"layers": [v], "bound": []})
    assert chk is None or not chk.fail, "%s is not provably exact here:\n  " % engine + "\n  ".join(chk.fail[:12])
    return out


def conv_layer_reference(x, w, b, res, relu):
    """one fused layer of cz_conv3x3_c128_bf16 in float64: x, res [B,90,128]; w [128,128,3,3], b [128] (folded).  The kernel adds
    the bias to the finished fp32 sum; without a residual it applies the ReLU and rounds to bf16 (RNE); with one it rounds the
    pre-residual sum to bf16 FIRST, adds the residual (both bf16, in fp32), applies the ReLU and rounds again.
    -> (result [B,90,128], the pre-residual sums, the values handed to the final rounding)"""
    B = x.shape[0]
    nchw = lambda t: t.detach().cpu().double().reshape(B, 9, 10, FILTERS).permute(0, 3, 1, 2)
    pre = _conv(nchw(x), w.detach().cpu().double()) + b.detach().cpu().double().view(1, -1, 1, 1)
    y = _round16(pre, BF16) + nchw(res) if res is not None else pre
    if relu:
        y = torch.relu(y)
    back = lambda t: t.permute(0, 2, 3, 1).reshape(B, 90, FILTERS)
    return back(_round16(y, BF16)), back(pre), back(y)


def conv_layer_check(x, w, b, res, relu, rounding=False):
    """conditions (a), (b) for one fused layer of cz_conv3x3_c128_bf16; -> list of failures.  (b): every partial sum of the
    products is an exact fp32 number, and so are the sum with the bias and the sum with the residual.  (a), rounding=False:
    the pre-residual sums and the results are bf16 values, both roundings are the identity.  rounding=True: they are NOT; on
    each rounding the kernel performs (the pre-residual one only with a residual) the reference meets at least 32 values rounded
    down, 32 rounded up and 32 exact ties"""
    exp, pre, y = conv_layer_reference(x, w, b, res, relu)
    tot = conv_layer_reference(x.abs(), w.abs(), b.abs(), None, False)[1]
    g = min(_granule(x.double()) * _granule(w.double()), _granule(b.double()))
    fail = []
    if not float(tot.max()) < 2.0 ** 24 * g:
        fail.append("sum |a w| + |b| = %.6g is not below 2^24 granules of %.3g" % (float(tot.max()), g))
    if not (torch.equal(pre.float().double(), pre) and torch.equal(y.float().double(), y)):
        fail.append("a sum with the bias or with the residual is no fp32 number")
    for name, t in (("pre-residual sum", pre), ("value handed to the final rounding", y)):
        if name.startswith("pre") and (rounding and res is None):
            continue
        r = _round16(t, BF16)
        if not rounding:
            if not torch.equal(r, t):
                fail.append("a %s is no bf16 value (largest %.6g)" % (name, float(t.abs().max())))
            continue
        q = t.abs() / _ulp(t, BF16)
        tie = (q - torch.floor(q)) == 0.5
        n = {"down": int((~tie & (r.abs() < t.abs())).sum()), "up": int((~tie & (r.abs() > t.abs())).sum()), "ties": int(tie.sum())}
        if min(n.values()) < 32:
            fail.append("%s: too few values off the bf16 grid: %s" % (name, n))
    return fail


def conv_layer_rounding_inputs():
    """-> (x, res, bias offsets [128]) for which both roundings of cz_conv3x3_c128_bf16 matter: integer activations 0 .. 40 (sums
    of a few hundred: bf16 keeps 8 bits) and eighths added to the dense family's integer biases"""
    return layer_activations(8, 0.3, 40), torch.roll(layer_activations(9, 0.3, 40), 1, 0), (torch.arange(FILTERS) % 8) / 8.0


def layer_activations(seed, density, top):
    """integer activations [185,90,128] for the per-layer kernels: 2 x 90 impulse rows (a single 1 at cell i, channel
    (7 i + k) mod 128, k = 0, 1) and 5 dense rows of integers 0 .. top"""
    gen = torch.Generator().manual_seed(seed)
    x = torch.zeros((185, 90, FILTERS))
    for k in range(2):
        for i in range(90):
            x[90 * k + i, i, (7 * i + k) % FILTERS] = 1.0
    x[180:] = torch.randint(0, top + 1, (5, 90, FILTERS), generator=gen) * (torch.rand((5, 90, FILTERS), generator=gen) < density)
    return x


def fc_inputs(B):
    """integer z [B,90,3] for the policy FC: a tenth of the entries 1 .. 3, one in 125 257, 259, 321 or 385 (9 significant bits: a bf16 hi + lo pair)"""
    gen = torch.Generator().manual_seed(B)
    z = torch.randint(1, 4, (B, 90, 3), generator=gen) * (torch.rand((B, 90, 3), generator=gen) < 0.1)
    big = torch.tensor([257.0, 385.0, 321.0, 259.0])[torch.randint(0, 4, (B, 90, 3), generator=gen)]
    z = torch.where(torch.rand((B, 90, 3), generator=gen) < 0.008, big, z.float())
    assert int((z[:, :, :2] > 256).sum()) > 0
    return z


def check_exact(module, x, engine, liveness=True):
    """The conditions under which `engine`'s output equals reference() bit for bit, all computed on the float64 reference:
    (a) every value the engine stores between layers (the trunk output included) survives a round trip through its storage
        format (bf16 / fp16 / a hi + lo pair of either / fp32), and every weight is exact in its operand format(s);
    (b) for every conv output  sum |a| |w| + |bias| + |residual| < 2^24 g,  g the granule of which every product, the bias and
        the residual are integer multiples: every partial sum, in any order, is then an exact fp32 number;
    (c) liveness: on a batch without impulse rows (unless liveness=False: a batch that is one of several an engine is fed, the
        caller then ORs "channels_alive" over them) at least a quarter of the last layer is non-zero and every channel of every
        layer is non-zero somewhere; for every impulse row every in-board neighbour of the impulse is non-zero after the
        first conv in some channel;
    mx_cross nets: every cross-term operand of the block-scaled MFMA sits on the E2M3 grid of its block.
    Round families: (a) reads "every value handed to the storage step is a finite exact fp32 number, and what is stored is
    the storage step's result (_store)"; a stored hi + lo pair is an fp32 number too, and mx6's fp32 last layer stays below
    65504; (b) is evaluated for every output element with that element's own granule; the E2M3 grid is not asserted.
    Raises AssertionError listing what fails; -> {"max_activation", "max_sum_over_2^24g", "alive_last", "channels_alive": bool [layers,128],
    which channels of which layer are non-zero somewhere in this batch (the caller ORs it over the batches an engine is fed)}."""
    chk = _Checks(engine)
    with torch.no_grad():
        out = _evaluate(module, x, engine, None, chk)
    cells = impulse_cells(torch.as_tensor(x).cpu())
    a0 = out["layers"][0]
    for r in (cells >= 0).nonzero().reshape(-1).tolist():
        y0, x0 = divmod(int(cells[r]), 10)
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                yy, xx = y0 + dy, x0 + dx
                if 0 <= yy < 9 and 0 <= xx < 10 and not bool((a0[r, :, yy, xx] != 0).any()):
                    chk.fail.append("impulse row %d: neighbour (%+d, %+d) is dead after the first conv" % (r, dy, dx))
    alive = float((out["layers"][-1] != 0).double().mean())
    if liveness and not bool((cells >= 0).any()):
        if alive < 0.25:
            chk.fail.append("only %.3f of the last layer is non-zero" % alive)
        for l, v in enumerate(out["layers"]):
            dead = int(((v != 0).sum(dim=(0, 2, 3)) == 0).sum())
            if dead:
                chk.fail.append("layer %d: %d output channels are zero everywhere" % (l, dead))
    assert not chk.fail, "%s is not provably exact here:\n  " % engine + "\n  ".join(chk.fail[:12])
    return {"max_activation": chk.max_act, "max_sum_over_2^24g": chk.max_ratio, "alive_last": alive,
            "channels_alive": torch.stack([(v != 0).sum(dim=(0, 2, 3)) > 0 for v in out["layers"]])}


# ---------------------------------------------------------------------------------------------------------------------
# the cases of the GPU test (tests/test_net_exact.py); tests/test_exactnets_cpu.py proves check_exact for every one of them
_PLAIN = [("sparse", 1, (0,)), ("sparse", 3, (0,)), ("sparse", 7, (0,)), ("dense", 1, tuple(range(DENSE_SEEDS)))]
CASES = {   # engine -> [(family, blocks, seeds)]
    "bf16": _PLAIN,
    "fp16": _PLAIN,
    "bf16x2": _PLAIN + [("lo", 1, (0,)), ("lo", 2, (0,))],
    "fp16x2": _PLAIN + [("lo", 1, (0,)), ("lo", 2, (0,)), ("lo_subnormal", 1, (0,))],
    "mx6": _PLAIN + [("mx_cross", 1, (0, 1)), ("mx_cross", 2, (0, 1, 2, 3))],      # seed % layers: the layer that carries w_lo
}
# the round family: 1 and 2 blocks per engine; seeds for which liveness holds and, over the engine's two nets and its batches,
# every case of round_cases() is met in every kind of layer that stores (tests/test_exactnets_cpu.py asserts both)
ROUND_SEEDS = {"bf16": (0, 0), "fp16": (0, 1), "bf16x2": (0, 0), "fp16x2": (1, 0), "mx6": (3, 4)}
for _e, _s in ROUND_SEEDS.items():
    CASES[_e] = CASES[_e] + [(ROUND_FAMILY[_e], 1, (_s[0],)), (ROUND_FAMILY[_e], 2, (_s[1],))]
SMALL_B = (1, 2, 3, 5)
LIVE_ROWS = 64      # dense rows every net is also run on: with them every channel of every layer is non-zero somewhere on the GPU


def gpu_batches(engine):
    """name -> planes: every batch tests/test_net_exact.py feeds a net of `engine` (the small batches are prefixes of these)"""
    g = GROUP[engine]
    return {"93": batch93(), "pairs of %d-position workgroups" % g: planes("pairs", max(SMALL_B), group=g),
            "dense": planes("dense", max(SMALL_B)), "live": planes("dense", LIVE_ROWS)}


def batch93():
    """the 90 impulses + 3 dense rows: a last workgroup with one live position for 2 and for 4 positions per workgroup"""
    return torch.cat([planes("impulses"), planes("dense", 3)])


def reference_engine(family, engine):
    """the engine whose reference serves `engine` on `family`: without lo halves (sparse, dense) every cross term of the strict
    engines is exactly zero and the plain float64 graph ("fp16") is the expected value of all five engines"""
    return "fp16" if family in ("sparse", "dense") else engine


# ---------------------------------------------------------------------------------------------------------------------
# comparison
def describe_mismatch(got, exp, what, x=None, group=1):
    """None when got == exp as values (+0 == -0, no NaN anywhere); else the failure message: the first differing
    (row, y, x, channel), got / expected, the number of differing elements, for an impulse row the (dy, dx) offset from the
    impulse, and the row's place in its workgroup.  got, exp: [B,90,C]"""
    got, exp = got.detach().cpu().double(), exp.detach().cpu().double()
    assert got.shape == exp.shape, (got.shape, exp.shape)
    if not bool(torch.isnan(got).any()) and torch.equal(got, exp):
        return None
    bad = (got != exp) | torch.isnan(got)
    r, cell, c = bad.nonzero()[0].tolist()
    msg = "%s: %d of %d elements differ (in %d rows); first at row %d (position %d of %d in its workgroup), y %d, x %d, channel %d: got %r, expected %r" % (
        what, int(bad.sum()), bad.numel(), int(bad.any(2).any(1).sum()), r, r % group + 1, group, cell // 10, cell % 10, c,
        float(got[r, cell, c]), float(exp[r, cell, c]))
    if x is not None:
        ic = int(impulse_cells(torch.as_tensor(x).cpu())[r])
        if ic >= 0:
            msg += "; impulse at y %d, x %d: offset (dy, dx) = (%+d, %+d)" % (ic // 10, ic % 10, cell // 10 - ic // 10, cell % 10 - ic % 10)
    return msg
