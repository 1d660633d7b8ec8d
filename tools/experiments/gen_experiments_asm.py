#!/usr/bin/env python3
"""Generates the hand-scheduled slab bodies of the trunk-kernel variants that were measured and not adopted:

  cz_experiments_slab_asm.inc   the variants of k_tower8_c128 (cz_trunk_experiments.h)
  cz_trunk_mx2_asm.inc          k_trunk_mx2_c128 (cz_trunk_mx2.h): slabMX2
  cz_trunk_mx12_asm.inc         k_trunk_mx12_c128 (cz_trunk_mx12.h): slabMX12

  usage: gen_experiments_asm.py [DIR] [--dma-place2 B|BC] [--ablate nodma,nobarrier]
DIR: where the three files go (default: next to this script; the two cz_trunk_mx*_asm.inc are not kept in git).  The product
kernels' bodies come from tools/gen_tower_asm.py, which this script imports for what the two share: emit, branchy, the k_tower8_c128
slab, the DMA-piece and register-range helpers, the ablation filter and the MX_* geometry.

One slab = 64 input channels of one 3x3 tap = 4 k-steps x 6 v_mfma_f32_32x32x16_bf16 per wave.
Issue plan (per wave, everything except the MFMAs sits in an MFMA's ~28-cycle issue shadow):
  k0  MFMAs on fragment set f0 | address math + ds_read_b128 x5 -> f2 (k-step 2 of this slab)
  k1  MFMAs on f1              | ... -> f3 (k-step 3)
  mid s_waitcnt vmcnt(4) ; s_barrier        (slab g+1 published, slab g-1's buffer free)
  k2  MFMAs on f2              | 4 x (m0 = LDS dst ; global_load_lds_dwordx4) of slab g+3, reads -> f0 (next slab k0)
  k3  MFMAs on f3              | reads -> f1 (next slab k1) ; s_waitcnt lgkmcnt(0)
Operands are named; the C++ side (cz_conv_kernel.h) binds them.  H = which 64-channel half of the tap.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gen_tower_asm import (ACC, MX_S_OFF, MX_XPLANE, MX_Y_OFF, MX_YPLANE, ablate_arg, branchy, dma_piece, emit, f16, kstep2, mfma, mx_ablated,  # noqa: E402
                           slab8, sub)


def kstep(Y, X, CA, OB0, OB1, AB, KEY, VB, wait, extras=None):
    ex = extras or [[], [], [], [], [], []]
    L = []
    if wait is not None:
        L.append("s_waitcnt lgkmcnt(%d)" % wait)
    L.append("v_xor_b32 %%[t0], %d, %%[%s0]" % (CA, KEY))
    L.append(mfma(0, 0, Y)); L += ex[0]
    L.append("v_xor_b32 %%[t1], %d, %%[%s1]" % (CA, KEY))
    L.append("v_xor_b32 %%[t2], %d, %%[%s2]" % (CA, KEY))
    L.append("v_lshl_add_u32 %%[t0], %%[t0], 4, %%[%s0]" % AB)
    L.append("v_lshl_add_u32 %%[t1], %%[t1], 4, %%[%s1]" % AB)
    L.append("v_lshl_add_u32 %%[t2], %%[t2], 4, %%[%s2]" % AB)
    L.append(mfma(0, 1, Y)); L += ex[1]
    L.append("ds_read_b128 %%[%sa0], %%[t0]" % X)
    L.append("ds_read_b128 %%[%sa1], %%[t1]" % X)
    L.append(mfma(1, 0, Y)); L += ex[2]
    L.append("ds_read_b128 %%[%sa2], %%[t2]" % X)
    L.append("ds_read_b128 %%[%sb0], %%[%s] offset:%d" % (X, VB, OB0))
    L.append(mfma(1, 1, Y)); L += ex[3]
    L.append("ds_read_b128 %%[%sb1], %%[%s] offset:%d" % (X, VB, OB1))
    L.append(mfma(2, 0, Y)); L += ex[4]
    L.append(mfma(2, 1, Y)); L += ex[5]
    return L


def slab(H):
    nab, nkey = ("ab", "key") if H == 0 else ("nab", "nkey")
    L = ["s_mov_b32 %[keep], m0"]
    L += kstep("f0", "f2", H * 8 + 4, 8192, 8704, "ab", "key", "vb", None)
    L += kstep("f1", "f3", H * 8 + 6, 12288, 12800, "ab", "key", "vb", None)
    L += ["s_waitcnt vmcnt(4)", "s_barrier"]
    dma = [["s_mov_b32 m0, %[ldst]", "s_nop 0", "global_load_lds_dwordx4 %[voff0], %[sbase]"],
           ["s_add_u32 m0, %[ldst], 0x1000", "s_nop 0", "global_load_lds_dwordx4 %[voff1], %[sbase]"],
           ["s_add_u32 m0, %[ldst], 0x2000", "s_nop 0", "global_load_lds_dwordx4 %[voff2], %[sbase]"],
           ["s_add_u32 m0, %[ldst], 0x3000", "s_nop 0", "global_load_lds_dwordx4 %[voff3], %[sbase]"], [], []]
    L += kstep("f2", "f0", (H ^ 1) * 8 + 0, 0, 512, nab, nkey, "vbn", 5, dma)
    L += kstep("f3", "f1", (H ^ 1) * 8 + 2, 4096, 4608, nab, nkey, "vbn", 5)
    L += ["s_waitcnt lgkmcnt(0)", "s_mov_b32 m0, %[keep]"]
    return L


def slabQ(hs):
    """Two-workgroups-per-CU variant (k_tower2x_c128): 8 KB slabs = 2 k-steps (32 input channels), 4 per tap.
    k0: f0 -> loads f1 (k1) ; vmcnt(2) + barrier ; k1: f1 -> f0 (k0 of the next slab; the next tap's addresses after
    the fourth slab) + 2 DMA pieces."""
    nab, nkey = ("nab", "nkey") if hs == 3 else ("ab", "key")
    L = ["s_mov_b32 %[keep], m0"]
    L += kstep2("f0", "f1", hs * 4 + 2, 4096, 4608, "ab", "key", "vb")
    L += ["s_waitcnt vmcnt(2)", "s_barrier"]
    dma = [["s_mov_b32 m0, %[ldst]", "s_nop 0", "global_load_lds_dwordx4 %[voff0], %[sbase]"], [],
           ["s_add_u32 m0, %[ldst], 0x1000", "s_nop 0", "global_load_lds_dwordx4 %[voff1], %[sbase]"], [], [], []]
    L += kstep2("f1", "f0", ((hs + 1) % 4) * 4, 0, 512, nab, nkey, "vbn", dma)
    L += ["s_mov_b32 m0, %[keep]"]
    return L


def slabSK(hs):
    """Skewed half-workgroup variant (k_towersk_c128): 4 positions / 8 waves, 8 KB slabs in an 8-slot ring.  Waves 0-3 (half A,
    positions 0-1) run SKEW slabs ahead of waves 4-7 (half B, positions 2-3) on the same slab sequence, so that one half's
    layer boundary (VALU) falls under the other half's MFMAs.  Only half A feeds the ring (its four waves move the whole 8 KB
    slab, two 1 KB pieces each, like the 2-position variant); half B skips the DMA with a scalar branch on its wave index %[wv] and finds its
    slabs published by the barriers it shares with A."""
    nab, nkey = ("nab", "nkey") if hs == 3 else ("ab", "key")
    L = ["s_mov_b32 %[keep], m0"]
    L += kstep2("f0", "f1", hs * 4 + 2, 4096, 4608, "ab", "key", "vb")
    L += ["s_waitcnt vmcnt(2)", "s_barrier"]
    dma = [["s_cmp_gt_u32 %[wv], 3", "s_cbranch_scc1 1f", "s_mov_b32 m0, %[ldst]", "s_nop 0",
            "global_load_lds_dwordx4 %[voff0], %[sbase]", "1:"], [],
           ["s_cmp_gt_u32 %[wv], 3", "s_cbranch_scc1 2f", "s_add_u32 m0, %[ldst], 0x1000", "s_nop 0",
            "global_load_lds_dwordx4 %[voff1], %[sbase]", "2:"], [], [], []]
    L += kstep2("f1", "f0", ((hs + 1) % 4) * 4, 0, 512, nab, nkey, "vbn", dma)
    L += ["s_mov_b32 m0, %[keep]"]
    return L


def kstepD(k):
    """Ring-free variant (k_towerd_c128): the weight fragments come straight from global memory (L1 / L2) into registers, so
    there is no LDS weight ring, no DMA and no per-slab barrier.  One macro per k-step, k = 0..23 (three taps = the period of
    the register rotation: activation fragments A0/A1 are requested from LDS one k-step ahead, weight fragments W0/W1/W2 from
    global two k-steps ahead).  k-step k computes on A[k%2], W[k%3], requests A[(k+1)%2] for k+1 (the next tap's row addresses
    when k is a tap's last k-step) and W[(k+2)%3] for k+2 (%[wn] = that k-step's 4 KB of the packed weights)."""
    a, an, w, wn = "A%d" % (k % 2), "A%d" % ((k + 1) % 2), "W%d" % (k % 3), "W%d" % ((k + 2) % 3)
    kk = k % 8
    ab, key = ("nab", "nkey") if kk == 7 else ("ab", "key")
    ca = ((kk + 1) % 8) * 2
    m = lambda i, j: "v_mfma_f32_32x32x16_bf16 %%[%s], %%[%sb%d], %%[%sa%d], %%[%s]" % (ACC[i][j], w, j, a, i, ACC[i][j])
    L = ["s_waitcnt lgkmcnt(0)", "s_waitcnt vmcnt(2)"]
    L.append("v_xor_b32 %%[t0], %d, %%[%s0]" % (ca, key))
    L.append(m(0, 0))
    L.append("v_xor_b32 %%[t1], %d, %%[%s1]" % (ca, key))
    L.append("v_xor_b32 %%[t2], %d, %%[%s2]" % (ca, key))
    L.append("v_lshl_add_u32 %%[t0], %%[t0], 4, %%[%s0]" % ab)
    L.append("v_lshl_add_u32 %%[t1], %%[t1], 4, %%[%s1]" % ab)
    L.append("v_lshl_add_u32 %%[t2], %%[t2], 4, %%[%s2]" % ab)
    L.append(m(0, 1))
    L.append("ds_read_b128 %%[%sa0], %%[t0]" % an)
    L.append("ds_read_b128 %%[%sa1], %%[t1]" % an)
    L.append(m(1, 0))
    L.append("ds_read_b128 %%[%sa2], %%[t2]" % an)
    L.append("global_load_dwordx4 %%[%sb0], %%[voff], %%[wn]" % wn)
    L.append(m(1, 1))
    L.append("global_load_dwordx4 %%[%sb1], %%[voff], %%[wn] offset:512" % wn)
    L.append(m(2, 0))
    L.append(m(2, 1))
    return L


ACCP = [["p%d%d" % (i, j) for j in range(4)] for i in range(3)]


def mfmaP(i, j, Y):
    return "v_mfma_f32_32x32x16_bf16 %%[%s], %%[%sb%d], %%[%sa%d], %%[%s]" % (ACCP[i][j], Y, j, Y, i, ACCP[i][j])


def kstepP(Y, X, CA, OB, AB, KEY, VB, extras=None, exp=0, zero_c=False):
    """Position-per-wave variant (one wave per SIMD, 3 cell tiles x 4 channel tiles = 12 MFMAs per k-step against
    7 fragment reads).  Two complete fragment sets: the k-step waits for its own set (requested during the previous
    k-step), then requests the other set for the next k-step, one ds_read_b128 per MFMA gap (a gap hides about five
    single-issue instructions; clustering the reads, or single-buffering the weight fragments behind counted
    waits, measured 4-7 % slower).  extras (LDS-DMA pieces, vmcnt-counted) go behind MFMAs 8..11."""
    ex = extras or []
    order = [(i, j) for j in range(4) for i in range(3)]
    L = [] if exp & 4 else ["s_waitcnt lgkmcnt(0)"]
    reads = ["ds_read_b128 %%[%sa%d], %%[t%d]" % (X, n, n) for n in range(3)]
    reads += ["ds_read_b128 %%[%sb%d], %%[%s] offset:%d" % (X, j, VB, OB + 512 * j) for j in range(4)]
    if exp & 8:
        reads = []
    for n in range(12):
        L.append(mfmaP(*order[n], Y))
        if n == 0 and not exp & 16:
            for m in range(3):
                L.append("v_xor_b32 %%[t%d], %d, %%[%s%d]" % (m, CA, KEY, m))
            for m in range(3):
                L.append("v_lshl_add_u32 %%[t%d], %%[t%d], 4, %%[%s%d]" % (m, m, AB, m))
        if 1 <= n <= len(reads):
            L.append(reads[n - 1])
        if 8 <= n < 8 + len(ex):
            L += ex[n - 8]
    if zero_c:   # first k-step of a layer: the accumulators start from an inline 0 instead of their old contents
        L = [l[:l.rindex(",")] + ", 0" if l.startswith("v_mfma") else l for l in L]
    return L


def slabP(H, exp=0, first=False):
    """k0: f0 -> loads f1 (k1) ; k1: f1 -> f0 (k2) ; vmcnt(4) + barrier ; k2: f0 -> f1 (k3) + 4 DMA pieces ;
    k3: f1 -> f0 (k0 of the next slab).  The DMA pieces share one lane-offset register; the 4 KB steps are four
    scalar bases (the 13-bit instruction offset cannot hold them)."""
    nab, nkey = ("ab", "key") if H == 0 else ("nab", "nkey")
    L = ["s_mov_b32 %[keep], m0"]
    L += kstepP("f0", "f1", H * 8 + 2, 4096, "ab", "key", "vb", exp=exp, zero_c=first)
    L += kstepP("f1", "f0", H * 8 + 4, 8192, "ab", "key", "vb", exp=exp)
    if not exp & 1:
        L += ["s_waitcnt vmcnt(4)", "s_barrier"]
    dma = [["s_mov_b32 m0, %[ldst]", "s_nop 0", "global_load_lds_dwordx4 %[voff0], %[sbase]"]]
    for q in (1, 2, 3):
        dma.append(["s_add_u32 m0, %%[ldst], 0x%x" % (q * 0x1000), "s_nop 0",
                    "global_load_lds_dwordx4 %%[voff0], %%[sbase%d]" % q])
    L += kstepP("f0", "f1", H * 8 + 6, 12288, "ab", "key", "vb", None if exp & 2 else dma, exp=exp)
    L += kstepP("f1", "f0", (H ^ 1) * 8 + 0, 0, nab, nkey, "vbn", exp=exp)
    L += ["s_mov_b32 m0, %[keep]"]
    return L


# ---- k_trunk_mx2_c128 (cz_trunk_mx2.h, round 6): the same arithmetic, LDS layout and slab format as k_trunk_mx_c128 with a 3 x 2
# register tile per wave and the K range of a layer split between the two waves of a pair (wave & 1 = kp handles the slabs
# 2 p + kp): 18 MFMAs per body instead of 9 with 20 + 5 LDS reads per body instead of 2 x (12 + 4) per 18 MFMAs, one barrier
# per PAIR of slabs, the partial sums exchanged once per layer.
MX2_AX = ["v[226:231]", "v[232:237]", "v[238:243]"]   # fp6 activation blocks of the three cell tiles
MX2_WX = ["v[244:249]", "v[250:255]"]                 # fp6 weight blocks of the two channel tiles (the body clobbers v226..v255)


MX2_ABLATIONS = ("nodma", "nobarrier")                # of the product's timing ablations, the two that mean something for these bodies


def slabMX2(first, layer_first=False, layer_last=False, ablate=(), dma_place="B"):
    """One body = one 16 KB slab (32 input channels of one tap) for a 3 cell x 2 channel tile: 12 fp16 MFMAs + 6 fp6 MFMAs.
    A wave sees two bodies per tap: `first` (quarter kp; the next body is quarter kp + 2 of the SAME tap: ab / key) and second
    (quarter kp + 2; the next body is quarter kp of the NEXT tap: nab / nkey) — the C++ side passes the right address operands
    as nab / nkey, and the quarter-dependent numbers as scalars (cba / cbb: 16-byte chunk of the next body's two k-steps; xo / yo:
    plane offsets of this body's fp6 blocks; kp8 = 8 kp: the tap's scale dword is shifted so that bytes 0 / 2 are this wave's
    quarters).  Channel tile j = 1 of the wave is 32 output channels = 512 / 256 / 128 bytes behind tile j = 0 in a slab's parts.
      A (k-step 0, set a0h* / w0*)  waits for its set (the 5 reads of set B may be in flight); requests this body's 12 fp6
                                    operand reads (+ 3 scale dwords in the first body of a tap)
      B (k-step 1, set a1h* / w1*)  every read of this wave has returned (lgkmcnt 0: the pair the DMAs below overwrite is no
                                    longer being read by anyone behind the barrier), its 4 DMA pieces have landed (vmcnt 0), barrier:
                                    the next pair is published; requests the next body's set A; 2 DMA pieces of the pair after next
      C (fp6, hard registers)       requests the next body's set B; the other 2 DMA pieces.
    layer_first: the first body of a layer — its DMAs were waited for when the previous layer drained, and the only vector-memory
    operations in flight are the epilogue's block-input stores, which the barrier need not wait for (no vmcnt wait).
    layer_last: the last body of a layer requests no operands (there is no next body: the activations are about to be replaced),
    so behind its barrier no wave reads the activation planes any more and the exchange may start without another barrier.
    Knobs: dma_place B (all four DMA pieces in step B) or BC; ablate: of the product's timing ablations, nodma and nobarrier."""
    f = lambda i, j, s: "v_mfma_f32_32x32x16_f16 %%[c%d%d], %%[w%d%d], %%[a%dh%d], %%[c%d%d]" % (i, j, s, j, s, i, i, j)
    mx = lambda i, j: ("v_mfma_scale_f32_32x32x64_f8f6f4 %%[c%d%d], %s, %s, %%[c%d%d], %%[ws%d], %%[sb%d] op_sel:[0,0,0] op_sel_hi:[0,%d,0] cbsz:2 blgp:2"
                       % (i, j, MX2_WX[j], MX2_AX[i], i, j, j, i, 0 if first else 1))
    L = ["s_mov_b32 %[keep], m0"]
    # ---- step A: the reads of THIS pair's buffers (the fp6 weight blocks and their scales) go out first, so that the counted
    # wait in front of the barrier covers them while the activation blocks may still be in flight
    L += ["s_waitcnt lgkmcnt(5)"]
    wreads = [["ds_read_b128 %s, %%[vb] offset:%d" % (sub(MX2_WX[j], 0, 3), 8192 + 512 * j), "ds_read_b64 %s, %%[vy] offset:%d" % (sub(MX2_WX[j], 4, 5), 256 * j),
               "ds_read_b32 %%[ws%d], %%[vs] offset:%d" % (j, 128 * j)] for j in range(2)]
    areads = [["v_add_u32 %%[t0], %%[xo], %%[xr%d]" % i, "v_add_u32 %%[t1], %%[yo], %%[yr%d]" % i,
               "ds_read_b128 %s, %%[t0]" % sub(MX2_AX[i], 0, 3), "ds_read_b64 %s, %%[t1]" % sub(MX2_AX[i], 4, 5)] for i in range(3)]
    sreads = (["v_lshrrev_b32 %%[t%d], 1, %%[yr%d]" % (k, k) for k in range(3)] +
              ["ds_read_b32 %%[sb%d], %%[t%d] offset:%d" % (k, k, MX_S_OFF) for k in range(3)]) if first else []
    fill = [wreads[0], wreads[1], areads[0], areads[1], areads[2], sreads]
    k = 0
    for i in range(3):
        for j in range(2):
            L += [f(i, j, 0)] + fill[k]
            k += 1
    behind_w = 6 + (3 if first else 0)      # reads issued behind the last read of the weight ring
    # ---- step B
    L += ["s_waitcnt lgkmcnt(%d)" % behind_w if layer_first else "s_waitcnt vmcnt(0) lgkmcnt(%d)" % (0 if layer_last else behind_w), "s_barrier"]
    # piece k of the wave: 1 KB at byte 8192 k + 16 tid of the 32 KB pair, to the same offset of the pair's two ring buffers; all four
    # right behind the barrier: they have the whole body to land (the next barrier waits for them)
    dma = [dma_piece("voff0")]
    dma += [["s_add_u32 m0, %%[ldst], 0x%x" % (0x2000 * k), "v_add_u32 %%[t3], 0x%x, %%[voff0]" % (0x2000 * k),
             "global_load_lds_dwordx4 %[t3], %[sbase]"] for k in (1, 2, 3)]

    def half(s, cb, woff, d, pre=None):
        """6 MFMAs of operand set s (fp16 k-step 1, or the fp6 step when s is None) with the requests of the next body's other
        set interleaved: address VALU, 5 reads; d: DMA pieces behind MFMAs 0..3"""
        X = 0 if s == 1 else 1          # the set being requested
        m = (lambda i, j: f(i, j, 1)) if s == 1 else (lambda i, j: mx(i, j))
        o = list(pre or [])
        rq = not layer_last
        o += [m(0, 0)] + d[0]
        o += ["v_xor_b32 %%[t%d], %%[%s], %%[nkey%d]" % (k, cb, k) for k in range(3)] if rq else []
        o += [m(0, 1)] + d[1]
        o += ["v_lshl_add_u32 %%[t%d], %%[t%d], 4, %%[nab%d]" % (k, k, k) for k in range(3)] if rq else []
        o += [m(1, 0)] + d[2]
        o += ["ds_read_b128 %%[a%dh0], %%[t0]" % X, "ds_read_b128 %%[a%dh1], %%[t1]" % X] if rq else []
        o += [m(1, 1)] + d[3]
        o += ["ds_read_b128 %%[a%dh2], %%[t2]" % X, "ds_read_b128 %%[w%d0], %%[vbn] offset:%d" % (X, woff)] if rq else []
        o += [m(2, 0)]
        o += ["ds_read_b128 %%[w%d1], %%[vbn] offset:%d" % (X, woff + 512)] if rq else []
        o += [m(2, 1)]
        return o
    none = [[], [], [], []]
    if dma_place == "B":    # one piece behind each of step B's first four MFMAs
        L += half(1, "cba", 0, dma)
        dC = none
    else:                   # "BC": two in step B, two in step C (the first version: 36 % slower than k_trunk_mx_c128)
        L += half(1, "cba", 0, [dma[0], [], dma[1], []])
        dC = [dma[2], [], dma[3], []]
    # ---- step C
    pre = ["s_waitcnt lgkmcnt(%d)" % (0 if layer_last else 5)] + (["v_lshrrev_b32 %%[sb%d], %%[kp8], %%[sb%d]" % (k, k) for k in range(3)] if first else [])
    L += half(None, "cbb", 4096, dC, pre)
    L += ["s_mov_b32 m0, %[keep]"]
    return mx_ablated(L, [a for a in ablate if a in MX2_ABLATIONS], 0)


# ---- k_trunk_mx12_c128 (cz_trunk_mx12.h, round 6): k_trunk_mx_c128's arithmetic, layout and slab format with TWELVE
# waves per workgroup (three per SIMD), two cell tiles per wave: the same MFMAs per slab and SIMD, a third wave to cover the waits.
MX12_AX = ["v[144:149]", "v[150:155]"]      # fp6 activation blocks of the two cell tiles
MX12_WX = "v[156:161]"                      # (the body clobbers v144..v161: below the 168 registers a wave of three per SIMD has)


def slabMX12(hs, pieces, layer_last=False):
    """slabMX for two cell tiles per wave: three steps of TWO MFMAs.  pieces: LDS-DMA pieces the wave issues per slab (waves 0-3: 2,
    waves 4-11: 1 — sixteen 1 KB pieces over twelve waves); its vmcnt wait lets exactly the previous body's pieces stay in flight."""
    nab, nkey = ("nab", "nkey") if hs == 3 else ("ab", "key")
    ca = ((hs + 1) % 4) * 4
    f = lambda i, w, a: "v_mfma_f32_32x32x16_f16 %%[c%d], %%[%s], %%[%s%d], %%[c%d]" % (i, w, a, i, i)
    mx = lambda i: ("v_mfma_scale_f32_32x32x64_f8f6f4 %%[c%d], %s, %s, %%[c%d], %%[ws], %%[sb%d] op_sel:[0,%d,0] op_sel_hi:[0,%d,0] cbsz:2 blgp:2"
                    % (i, MX12_WX, MX12_AX[i], i, i, hs & 1, hs >> 1))
    xo, yo = hs * 2 * MX_XPLANE, MX_Y_OFF + hs * 2 * MX_YPLANE
    L = ["s_mov_b32 %[keep], m0"]
    # step A
    L += ["s_waitcnt lgkmcnt(3)", f(0, "w0", "a0h")]
    L += ["ds_read_b128 %s, %%[xr0] offset:%d" % (sub(MX12_AX[0], 0, 3), xo), "ds_read_b64 %s, %%[yr0] offset:%d" % (sub(MX12_AX[0], 4, 5), yo),
          "ds_read_b128 %s, %%[xr1] offset:%d" % (sub(MX12_AX[1], 0, 3), xo), "ds_read_b64 %s, %%[yr1] offset:%d" % (sub(MX12_AX[1], 4, 5), yo)]
    nc = 7
    if hs == 0:
        L += ["v_lshrrev_b32 %[t0], 1, %[yr0]", "v_lshrrev_b32 %[t1], 1, %[yr1]"]
        L += ["ds_read_b32 %%[sb%d], %%[t%d] offset:%d" % (i, i, MX_S_OFF) for i in range(2)]
        nc = 9
    L += [f(1, "w0", "a0h")]
    L += ["ds_read_b128 %s, %%[vb] offset:8192" % sub(MX12_WX, 0, 3), "ds_read_b64 %s, %%[vy]" % sub(MX12_WX, 4, 5), "ds_read_b32 %[ws], %[vs]"]
    # step B
    if layer_last:
        L += ["s_waitcnt vmcnt(%d) lgkmcnt(0)" % pieces, "s_barrier", f(0, "w1", "a1h"), f(1, "w1", "a1h")]
    else:
        L += ["s_waitcnt vmcnt(%d)" % pieces, "s_barrier", "s_waitcnt lgkmcnt(%d)" % nc]
        L += [f(0, "w1", "a1h")]
        L += ["v_xor_b32 %%[t%d], %d, %%[%s%d]" % (i, ca, nkey, i) for i in range(2)]
        L += ["v_lshl_add_u32 %%[t%d], %%[t%d], 4, %%[%s%d]" % (i, i, nab, i) for i in range(2)]
        L += [f(1, "w1", "a1h")]
        L += ["ds_read_b128 %[a0h0], %[t0]", "ds_read_b128 %[a0h1], %[t1]", "ds_read_b128 %[w0], %[vbn]"]
    # step C
    L += [] if layer_last else ["s_waitcnt lgkmcnt(3)"]
    L += [mx(0)]
    if not layer_last:
        L += ["v_xor_b32 %%[t%d], %d, %%[%s%d]" % (i, ca + 2, nkey, i) for i in range(2)]
        L += ["v_lshl_add_u32 %%[t%d], %%[t%d], 4, %%[%s%d]" % (i, i, nab, i) for i in range(2)]
    L += dma_piece("voff0") + (dma_piece("voff1", 0x3000) if pieces == 2 else [])
    L += [mx(1)]
    L += [] if layer_last else ["ds_read_b128 %[a1h0], %[t0]", "ds_read_b128 %[a1h1], %[t1]", "ds_read_b128 %[w1], %[vbn] offset:4096"]
    L += ["s_mov_b32 m0, %[keep]"]
    return L


def write_inc(directory, name, txt):
    with open(os.path.join(directory, name), "w") as f:
        f.write("// GENERATED by tools/experiments/gen_experiments_asm.py — do not edit.  See that script for the issue plan.\n" + txt)


def mx2_inc(**knobs):
    c0 = ("%[c00],", "%[c01],")
    txt = "// k_trunk_mx2_c128: 8 waves / 2 positions, 3 x 2 tiles per wave, K split between the waves of a pair: 12 fp16 + 6 fp6 MFMAs per body\n"
    for name, first in (("A", True), ("B", False)):
        txt += emit("MX2_BODY_%s" % name, slabMX2(first, **knobs)) + "\n"
        txt += emit("MX2_SKIP0_%s" % name, branchy(slabMX2(first, **knobs), c0)) + "\n"
    txt += "// the first body of a layer (tap 0: with the skip; no vmcnt wait) and the last (no operand requests)\n"
    txt += emit("MX2_SKIP0_A_FIRST", branchy(slabMX2(True, layer_first=True, **knobs), c0)) + "\n"
    return txt + emit("MX2_BODY_B_LAST", slabMX2(False, layer_last=True, **knobs)) + "\n"


def mx12_inc():
    txt = "// k_trunk_mx12_c128: 12 waves / 2 positions, 2 cell tiles per wave: 4 fp16 + 2 fp6 MFMAs per slab and wave\n"
    for hs in range(4):
        txt += emit("MX12_SKIP0_P2_Q%d" % hs, branchy(slabMX12(hs, 2), ("%[c0],",))) + "\n"    # waves 0-3: two DMA pieces, dy = -1 skip of tile 0
        txt += emit("MX12_SLAB_P2_Q%d" % hs, slabMX12(hs, 2)) + "\n"
        txt += emit("MX12_SLAB_P1_Q%d" % hs, slabMX12(hs, 1)) + "\n"
    return txt + emit("MX12_SLAB_P2_Q3_LAST", slabMX12(3, 2, layer_last=True)) + "\n" + emit("MX12_SLAB_P1_Q3_LAST", slabMX12(3, 1, layer_last=True)) + "\n"


def main():
    ap = argparse.ArgumentParser(description="writes cz_experiments_slab_asm.inc, cz_trunk_mx2_asm.inc and cz_trunk_mx12_asm.inc")
    ap.add_argument("directory", nargs="?", default=os.path.dirname(os.path.abspath(__file__)))
    ap.add_argument("--dma-place2", default="B", choices=("B", "BC"), help="k_trunk_mx2_c128: where a body's four DMA pieces go")
    ap.add_argument("--ablate", default=(), type=ablate_arg(MX2_ABLATIONS), help="k_trunk_mx2_c128: nodma, nobarrier (comma separated)")
    a = ap.parse_args()
    write_inc(a.directory, "cz_trunk_mx2_asm.inc", mx2_inc(ablate=a.ablate, dma_place=a.dma_place2))
    write_inc(a.directory, "cz_trunk_mx12_asm.inc", mx12_inc())
    txt = emit("TW_SLAB_ASM_H0", slab(0)) + "\n" + emit("TW_SLAB_ASM_H1", slab(1))
    txt += "\n// skewed half-workgroup variant (4 positions / 8 waves, 8 KB slabs, 8-slot ring fed by waves 0-3), bf16 and fp16\n"
    for hs in range(4):
        txt += emit("TWS_SLAB_ASM_Q%d" % hs, slabSK(hs)) + "\n" + emit("TWSF_SLAB_ASM_Q%d" % hs, f16(slabSK(hs))) + "\n"
    txt += "\n// ring-free variant: weight fragments from global memory, one macro per k-step of the 24-k-step rotation period, bf16 and fp16\n"
    for k in range(24):
        txt += emit("TWD_KSTEP_%d" % k, kstepD(k)) + "\n" + emit("TWDF_KSTEP_%d" % k, f16(kstepD(k))) + "\n"
    txt += "\n// position-per-wave variant (4 waves, 3 cell tiles x 4 channel tiles each, two fragment sets)\n"
    txt += emit("TWP_SLAB_ASM_H0", slabP(0)) + "\n" + emit("TWP_SLAB_ASM_H1", slabP(1))
    txt += "\n" + emit("TWP_SLAB_ASM_FIRST", slabP(0, first=True))
    # zero-work elasticity experiment (tower_skip_ubench.hip): k_tower8_c128's slab with the MFMAs of the wave's third cell tile
    # removed (a third of the MFMAs; wrong results, timing only) — what does issuing fewer MFMAs buy under the power governor?
    drop = lambda L: [l for l in L if not (l.startswith("v_mfma") and ("%[c20]" in l or "%[c21]" in l))]
    txt += "\n// k_tower8_c128 slab without the third cell tile's MFMAs (timing experiment)\n"
    txt += emit("TW8F_SKIP_ASM_H0", f16(drop(slab8(0)))) + "\n" + emit("TW8F_SKIP_ASM_H1", f16(drop(slab8(1)))) + "\n"
    txt += emit("TW8_SKIP_ASM_H0", drop(slab8(0))) + "\n" + emit("TW8_SKIP_ASM_H1", drop(slab8(1))) + "\n"
    if os.environ.get("CZ_TP_EXP"):   # timing experiments only (wrong results): 1 = no barrier, 2 = no DMA, 4 = no LDS waits, 8 = no fragment reads, 16 = no address math
        e = int(os.environ["CZ_TP_EXP"])
        txt = txt.replace("#define TWP_SLAB_ASM_H", "#define TWP_REAL_SLAB_ASM_H")
        txt += emit("TWP_SLAB_ASM_H0", slabP(0, e)) + "\n" + emit("TWP_SLAB_ASM_H1", slabP(1, e))
        txt += "\n" + emit("TWP_SLAB_ASM_FIRST", slabP(0, e, first=True))
    write_inc(a.directory, "cz_experiments_slab_asm.inc", txt)
    print("wrote cz_experiments_slab_asm.inc (%d instructions per slab), cz_trunk_mx2_asm.inc (%d per body), cz_trunk_mx12_asm.inc in %s" %
          (len(slab(0)), len(slabMX2(False)), a.directory))


if __name__ == "__main__":
    main()
