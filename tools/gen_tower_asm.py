#!/usr/bin/env python3
"""Generates the hand-scheduled slab bodies of the product trunk kernels:

  cchess_zero_amd/csrc/cz_tower_slab_asm.inc   k_tower8_c128 (cz_conv_kernel.h): 4 positions / 8 waves, 16-bit operands
  cchess_zero_amd/csrc/cz_trunk_split_asm.inc  k_trunk_split_c128 (cz_trunk_split.h): 2 positions / 8 waves, every
                                               operand split into two 16-bit halves, three MFMAs per product
  cchess_zero_amd/csrc/cz_trunk_mx_asm.inc     k_trunk_mx_c128 (cz_trunk_mx.h): the same tiling, fp16 hi halves + both cross
                                               terms on one block-scaled fp6 MFMA (1.5 MFMA-equivalents per product)

k_tower8_c128: one slab = 64 input channels of one 3x3 tap = 4 k-steps x 6 v_mfma_f32_32x32x16 per wave; two fragment
sets; each k-step first waits for its own set (the partner wave on the SIMD covers the wait), then interleaves its 6
MFMAs with the 5 ds_read_b128 of the next k-step; the LDS-DMA pieces of slab g+3 go out behind the barrier in the middle
of slab g.  Everything except the MFMAs sits in an MFMA's issue shadow.  Operands are named; the C++ side binds them.
(The bodies of the variants that were measured and not adopted: tools/experiments/gen_experiments_asm.py, which imports the
helpers and the MX_* geometry below.)

  usage: gen_tower_asm.py [DIR] [--ablate a,b,...] [--dma-place C|B0|B0C0|Cend] [--body-pad none|all|q0]
With no argument it writes the three committed files, and the committed files are what it writes with no option: the options
are the experiment knobs of slabMX (tools/experiments/mx_ablate.sh passes them, with a DIR of its own).  Nothing is read from the
environment.
"""
import argparse
import os

ACC = [["c00", "c01"], ["c10", "c11"], ["c20", "c21"]]


def sub(r, lo, hi):
    """registers lo .. hi of the hard register range r, written v[a:b]"""
    a = int(r[2:].split(":")[0])
    return "v[%d:%d]" % (a + lo, a + hi)


def dma_piece(voff, off=None):
    """one LDS-DMA piece of a wave: m0 = its LDS destination (ldst, + off bytes), the wait state m0 needs, 1 KB from sbase + voff"""
    m0 = "s_mov_b32 m0, %[ldst]" if off is None else "s_add_u32 m0, %%[ldst], 0x%x" % off
    return [m0, "s_nop 0", "global_load_lds_dwordx4 %%[%s], %%[sbase]" % voff]


def f16(L):
    return [l.replace("v_mfma_f32_32x32x16_bf16", "v_mfma_f32_32x32x16_f16") for l in L]


def branchy(L, accs=("%[c00],", "%[c01],")):
    """the dy = -1 taps: a cell group whose FIRST row tile holds only rank-0 cells and padding rows (groups 0 and 1) reads the zero
    row for all of that tile's inputs and does not issue its MFMAs (accs: their accumulators): a scalar branch around each of them
    on VCC (set from the wave-uniform 32-bit %[skipm] at the top of the body; nothing in the body writes VCC).  One body for all
    waves — a wave-dependent choice between two bodies makes hipcc copy / spill the accumulators where the paths join."""
    out = ["s_cmp_lg_u32 %[skipm], 0", "s_cselect_b64 vcc, -1, 0"]
    for l in L:
        if l.startswith("v_mfma") and any(l.split()[1] == a for a in accs):
            out += ["s_cbranch_vccnz 1f", l, "1:"]
        else:
            out.append(l)
    return out


def branchy2(L):
    """the general form: bit 0 of %[skipm] skips the wave's FIRST row tile (c00, c01: branch on VCC, set once at the top), bit 1 its
    SECOND (c10, c11: s_bitcmp1 + branch on SCC in front of each MFMA; nothing between the two reads or writes SCC)"""
    out = ["s_bitcmp1_b32 %[skipm], 0", "s_cselect_b64 vcc, -1, 0"]
    for l in L:
        acc = l.split()[1] if l.startswith("v_mfma") else ""
        if acc in ("%[c00],", "%[c01],"):
            out += ["s_cbranch_vccnz 1f", l, "1:"]
        elif acc in ("%[c10],", "%[c11],"):
            out += ["s_bitcmp1_b32 %[skipm], 1", "s_cbranch_scc1 2f", l, "2:"]
        else:
            out.append(l)
    return out


def mfma(i, j, Y):
    return "v_mfma_f32_32x32x16_bf16 %%[%s], %%[%sb%d], %%[%sa%d], %%[%s]" % (ACC[i][j], Y, j, Y, i, ACC[i][j])


def kstep2(Y, X, CA, OB0, OB1, AB, KEY, VB, extras=None):
    """8-wave variant: two fragment sets, each k-step first waits for its own set (the partner wave on the SIMD
    covers the wait), then interleaves its 6 MFMAs with the 5 reads of the next k-step."""
    ex = extras or [[], [], [], [], [], []]
    L = ["s_waitcnt lgkmcnt(0)"]
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


def slab8(H):
    """k0: f0 -> loads f1 (k1) ; k1: f1 -> f0 (k2) ; mid ; k2: f0 -> f1 (k3) + 2 DMA pieces ; k3: f1 -> f0 (next slab k0)."""
    nab, nkey = ("ab", "key") if H == 0 else ("nab", "nkey")
    L = ["s_mov_b32 %[keep], m0"]
    L += kstep2("f0", "f1", H * 8 + 2, 4096, 4608, "ab", "key", "vb")
    L += kstep2("f1", "f0", H * 8 + 4, 8192, 8704, "ab", "key", "vb")
    L += ["s_waitcnt vmcnt(2)", "s_barrier"]
    dma = [dma_piece("voff0"), [], dma_piece("voff1", 0x2000), [], [], []]
    L += kstep2("f0", "f1", H * 8 + 6, 12288, 12800, "ab", "key", "vb", dma)
    L += kstep2("f1", "f0", (H ^ 1) * 8 + 0, 0, 512, nab, nkey, "vbn")
    L += ["s_mov_b32 m0, %[keep]"]
    return L


def kstepX(Y, X, CA, OB, AB, KEY, VB, LO, extras=None):
    """Split-operand variant (k_trunk_split_c128): a wave owns 3 cell tiles x 1 channel tile.  Fragment set = activation
    hi/lo halves of the 3 cell tiles (ah0-2, al0-2; the lo half of a row lives LO bytes behind its hi half) + the weight
    tile's hi/lo halves (wh, wl).  9 MFMAs per k-step: c_i += wh*ah_i ; c_i += wl*ah_i ; c_i += wh*al_i (lo*lo is below
    fp32 resolution of the sum and is dropped) — the three products of one accumulator are three MFMAs apart.  The 8 reads of
    the next k-step's set are spread over the first six MFMA shadows; extras (LDS-DMA pieces) follow."""
    ex = extras or [[] for _ in range(9)]
    m = lambda i, w, a: "v_mfma_f32_32x32x16_bf16 %%[c%d], %%[%s%s], %%[%s%s%d], %%[c%d]" % (i, Y, w, Y, a, i, i)
    L = ["s_waitcnt lgkmcnt(0)"]
    L.append("v_xor_b32 %%[t0], %d, %%[%s0]" % (CA, KEY))
    L.append(m(0, "wh", "ah")); L += ex[0]
    L.append("v_xor_b32 %%[t1], %d, %%[%s1]" % (CA, KEY))
    L.append("v_xor_b32 %%[t2], %d, %%[%s2]" % (CA, KEY))
    L.append("v_lshl_add_u32 %%[t0], %%[t0], 4, %%[%s0]" % AB)
    L.append("v_lshl_add_u32 %%[t1], %%[t1], 4, %%[%s1]" % AB)
    L.append("v_lshl_add_u32 %%[t2], %%[t2], 4, %%[%s2]" % AB)
    L.append(m(1, "wh", "ah")); L += ex[1]
    L.append("ds_read_b128 %%[%sah0], %%[t0]" % X)
    L.append("ds_read_b128 %%[%sal0], %%[t0] offset:%d" % (X, LO))
    L.append(m(2, "wh", "ah")); L += ex[2]
    L.append("ds_read_b128 %%[%sah1], %%[t1]" % X)
    L.append("ds_read_b128 %%[%sal1], %%[t1] offset:%d" % (X, LO))
    L.append(m(0, "wl", "ah")); L += ex[3]
    L.append("ds_read_b128 %%[%sah2], %%[t2]" % X)
    L.append("ds_read_b128 %%[%sal2], %%[t2] offset:%d" % (X, LO))
    L.append(m(1, "wl", "ah")); L += ex[4]
    L.append("ds_read_b128 %%[%swh], %%[%s] offset:%d" % (X, VB, OB))
    L.append("ds_read_b128 %%[%swl], %%[%s] offset:%d" % (X, VB, OB + 8192))
    L.append(m(2, "wl", "ah")); L += ex[5]
    L.append(m(0, "wh", "al")); L += ex[6]
    L.append(m(1, "wh", "al")); L += ex[7]
    L.append(m(2, "wh", "al")); L += ex[8]
    return L


def slabX(hs, LO):
    """One 16 KB slab = 32 input channels of one tap, hi halves (8 KB) then lo halves (8 KB) = 2 k-steps, 4 slabs per tap.
    k0: f0 -> loads f1 (k1) ; vmcnt(2) + barrier (slab g+1 published, slab g-1's buffer free) ; k1: f1 -> loads f0 (k0 of the
    next slab; the next tap's addresses after the fourth slab) + the wave's 2 DMA pieces of slab g+3."""
    nab, nkey = ("nab", "nkey") if hs == 3 else ("ab", "key")
    L = ["s_mov_b32 %[keep], m0"]
    L += kstepX("f0", "f1", hs * 4 + 2, 4096, "ab", "key", "vb", LO)
    L += ["s_waitcnt vmcnt(2)", "s_barrier"]
    dma = [[] for _ in range(9)]
    dma[5], dma[7] = dma_piece("voff0"), dma_piece("voff1", 0x2000)
    L += kstepX("f1", "f0", ((hs + 1) % 4) * 4, 0, nab, nkey, "vbn", LO, dma)
    L += ["s_mov_b32 m0, %[keep]"]
    return L


XS_LO_OFF = 181 * 256   # cz_trunk_split.h: XSGeo::LO_OFF (180 activation rows + the zero row)

# ---- k_trunk_mx_c128 (cz_trunk_mx.h): a*w = a_hi*w_hi on two fp16 MFMAs per 32 input channels + BOTH cross terms of those 32
# channels on ONE block-scaled fp6 MFMA (v_mfma_scale_f32_32x32x64_f8f6f4, 8 passes): 9 MFMAs per slab and wave instead of 18.
MX_XPLANE, MX_YPLANE = 224 * 16, 224 * 8      # MXGeo: one plane per 16-channel group, 224 entries (180 cells + the zero aliases)
MX_Y_OFF, MX_S_OFF = 8 * MX_XPLANE, 8 * MX_XPLANE + 8 * MX_YPLANE
MX_SLAB = 16384                               # MXGeo::SLAB_BYTES: one slot of the ring of four
MX_AX = ["v[232:237]", "v[238:243]", "v[244:249]"]   # fp6 activation blocks of the three cell tiles: loaded and consumed inside
MX_WX = "v[250:255]"                                  # one slab body, so they are hard registers (the body clobbers v232..v255)
MX_HI_ROWB = 272                              # MXGeo::HI_ROWB: a hi row's 256 bytes + 16 of padding; chunk c at 16 c, no swizzle


def mx_hi_chunks(hs):
    """the 16-byte chunks (lower k-half; the upper reads the next one) of the two fp16 operand sets that body hs requests: the NEXT
    slab's k-steps 0 and 1, i.e. input channels 32 (hs + 1) .. + 31 of the tap, after the tap's last slab channels 0 .. 31"""
    ca = ((hs + 1) % 4) * 4
    return ca, ca + 2


def mx_body_bytes(L):
    """encoded length of a body of slabMX: scalar instructions 4 bytes (8 with a literal: constants outside 0..64), the block-scaled
    MFMA 16, every other MFMA, LDS read and LDS-DMA 8 (checked once against the assembler's listing of the built kernel)"""
    n = 0
    for l in L:
        op = l.split()[0]
        if op.startswith("s_"):
            lit = op == "s_add_u32" and int(l.split()[-1], 16) > 64
            n += 8 if lit else 4
        else:
            n += 16 if op.startswith("v_mfma_scale") else 8
    return n


MX_ABLATIONS = ("nolgkmwait", "novmwait", "nobarrier", "bar2", "noc", "nomx", "nodma", "nohi")


def ablate_arg(known=MX_ABLATIONS):
    """argparse type of an --ablate option: "a,b" -> ("a", "b"); a name that is not one of `known` is an error"""
    def parse(s):
        names = tuple(x for x in s.split(",") if x)
        bad = [x for x in names if x not in known]
        if bad:
            raise argparse.ArgumentTypeError("unknown ablation %s (known: %s)" % (", ".join(bad), ", ".join(known)))
        return names
    return parse


def mx_ablated(L, ab, hs):
    """timing ablations of a body of quarter hs (tools/experiments/mx_ablate.sh; wrong results): ab = any of nolgkmwait, novmwait,
    nobarrier, bar2 (barrier in every other slab), noc (no fp6 operand reads), nomx (no fp6 MFMAs), nodma, nohi (no fp16 operand reads)"""
    if "nobarrier" in ab or ("bar2" in ab and hs % 2 == 1):
        L = [l for l in L if l != "s_barrier"]
    if "noc" in ab:
        L = [l for l in L if not (l.startswith("ds_read") and ("v[2" in l or "%[ws]" in l or "%[sb" in l))]
        L = [l.replace("lgkmcnt(12)", "lgkmcnt(0)").replace("lgkmcnt(9)", "lgkmcnt(0)") for l in L]
    if "nohi" in ab:
        L = [l for l in L if not (l.startswith("ds_read_b128 %[a") or l.startswith("ds_read_b128 %[w"))]
        L = [l.replace("lgkmcnt(4)", "lgkmcnt(0)") for l in L]
    if "nomx" in ab:
        L = [l for l in L if not l.startswith("v_mfma_scale")]
    if "nolgkmwait" in ab:    # operands are never waited for: what perfect latency hiding of the LDS reads would buy (same LDS traffic)
        L = [l for l in L if not l.startswith("s_waitcnt lgkmcnt")]
    if "novmwait" in ab:      # the DMAs are issued but never waited for: issue cost vs waiting for the data
        L = [l.replace("s_waitcnt vmcnt(2)", "s_nop 0") for l in L]
    if "nodma" in ab:
        L = [l for l in L if not l.startswith("global_load_lds")]
        L = [l.replace("s_waitcnt vmcnt(2)", "s_nop 0") for l in L]
    return L


def slabMX(hs, layer_last=False, ablate=(), dma_place="C", body_pad="none"):
    """One 16 KB slab = 32 input channels of one tap: [fp16 hi: 2 k-steps x 2 halves x 128 co x 8][fp6 blocks: X 2 x 128 x 16 B,
    Y 2 x 128 x 8 B][E8M0 scale dwords 2 x 128].  Three steps of three MFMAs; operands are requested TWO steps ahead:
      A (k-step 0, set a0*/w0)  waits for its set (the next step's 4 reads may be in flight), requests this slab's fp6 set
      B (k-step 1, set a1*/w1)  vmcnt(2) + barrier first (slab g+1 published, slab g-1's buffer free), requests the NEXT slab's
                                set A (after the fourth slab of a tap: at the next tap's addresses)
      C (fp6, hard registers)   requests the next slab's set B, issues the wave's 2 DMA pieces of slab g+3.
    36 slabs per layer = a multiple of 4: slab g lives in ring slot g & 3 = hs, so the slots are immediates: the weight reads carry
    them in their offset fields (vb / vy / vs are the wave's addresses in slot 0), the DMA adds its slot to ldst (slot 0 + 1 KB per
    wave); from slab to slab only the DMA's global source moves (tests/test_mx_slab_plan_cpu.py walks a layer of these bodies).
    layer_last (round 6): the LAST slab of a layer requests no operands (the activations are about to be replaced) and waits
    for all of its LDS reads in front of its barrier — behind it no wave reads the activation planes any more, so the epilogue
    needs no barrier of its own in front.
    The fp16 hi rows sit on a padded stride (MXGeo::HI_ROWB = 272 B = 68 dwords: conflict-free without a swizzle), so a row's chunk is
    an immediate as well: ab / nab are the lane's row (or its zero alias) + 16 B for the upper k-half, the reads add 16 * chunk.  The
    tap's scale addresses come in as sr0..2.  A body holds no VALU instruction besides its MFMAs.
    The experiment knobs (the committed bodies are the defaults): ablate (mx_ablated), dma_place (where the wave's two LDS-DMA pieces
    go: C, B0, B0C0, Cend), body_pad (none, all, q0: below)."""
    nab = "nab" if hs == 3 else "ab"
    ca, cb = mx_hi_chunks(hs)
    f = lambda i, w, a: "v_mfma_f32_32x32x16_f16 %%[c%d], %%[%s], %%[%s%d], %%[c%d]" % (i, w, a, i, i)
    hi = lambda s, i, c: "ds_read_b128 %%[a%dh%d], %%[%s%d] offset:%d" % (s, i, nab, i, 16 * c)
    mx = lambda i: ("v_mfma_scale_f32_32x32x64_f8f6f4 %%[c%d], %s, %s, %%[c%d], %%[ws], %%[sb%d] op_sel:[0,%d,0] op_sel_hi:[0,%d,0] cbsz:2 blgp:2"
                    % (i, MX_WX, MX_AX[i], i, i, hs & 1, hs >> 1))
    xo, yo = hs * 2 * MX_XPLANE, MX_Y_OFF + hs * 2 * MX_YPLANE
    slot, nslot, dslot = hs * MX_SLAB, ((hs + 1) % 4) * MX_SLAB, ((hs + 3) % 4) * MX_SLAB     # this slab's, the next slab's, the DMA's
    L = ["s_mov_b32 %[keep], m0"]
    # step A
    L += ["s_waitcnt lgkmcnt(4)", f(0, "w0", "a0h")]
    L += ["ds_read_b128 %s, %%[xr0] offset:%d" % (sub(MX_AX[0], 0, 3), xo), "ds_read_b64 %s, %%[yr0] offset:%d" % (sub(MX_AX[0], 4, 5), yo),
          "ds_read_b128 %s, %%[xr1] offset:%d" % (sub(MX_AX[1], 0, 3), xo), "ds_read_b64 %s, %%[yr1] offset:%d" % (sub(MX_AX[1], 4, 5), yo)]
    L += [f(1, "w0", "a0h")]
    L += ["ds_read_b128 %s, %%[xr2] offset:%d" % (sub(MX_AX[2], 0, 3), xo), "ds_read_b64 %s, %%[yr2] offset:%d" % (sub(MX_AX[2], 4, 5), yo)]
    nc = 9
    if hs == 0:   # the tap's activation scales: one dword per cell = the four 32-channel quarters' E8M0 bytes of this lane's half
        L += ["ds_read_b32 %%[sb%d], %%[sr%d] offset:%d" % (i, i, MX_S_OFF) for i in range(3)]
        nc = 12
    L += [f(2, "w0", "a0h")]
    L += ["ds_read_b128 %s, %%[vb] offset:%d" % (sub(MX_WX, 0, 3), slot + 8192), "ds_read_b64 %s, %%[vy] offset:%d" % (sub(MX_WX, 4, 5), slot),
          "ds_read_b32 %%[ws], %%[vs] offset:%d" % slot]
    # step B
    if layer_last:
        L += ["s_waitcnt vmcnt(2) lgkmcnt(0)", "s_barrier"]
        L += [f(0, "w1", "a1h"), f(1, "w1", "a1h"), f(2, "w1", "a1h")]
    else:
        L += ["s_waitcnt vmcnt(2)", "s_barrier", "s_waitcnt lgkmcnt(%d)" % nc]
        L += [f(0, "w1", "a1h")]
        L += [f(1, "w1", "a1h")]
        L += [hi(0, 0, ca), hi(0, 1, ca)]
        L += [f(2, "w1", "a1h")]
        L += [hi(0, 2, ca), "ds_read_b128 %%[w0], %%[vb] offset:%d" % nslot]
    # step C
    dma1, dma2 = dma_piece("voff0", dslot), dma_piece("voff1", dslot + 0x2000)
    place = dma_place
    if place == "B0":       # both right behind the barrier
        i = L.index("s_barrier") + 1
        L[i:i] = dma1 + dma2
    elif place == "B0C0":   # one behind the barrier, one at the top of step C
        i = L.index("s_barrier") + 1
        L[i:i] = dma1
    L += [] if layer_last else ["s_waitcnt lgkmcnt(4)"]
    if place == "B0C0":
        L += dma2
    L += [mx(0)]
    if place == "C":
        L += dma1
    L += [mx(1)]
    L += [] if layer_last else [hi(1, 0, cb), hi(1, 1, cb)]
    if place == "C":
        L += dma2
    L += [mx(2)]
    L += [] if layer_last else [hi(1, 2, cb), "ds_read_b128 %%[w1], %%[vb] offset:%d" % (nslot + 4096)]
    if place == "Cend":
        L += dma1 + dma2
    # body_pad: one s_nop 0 that makes every body a multiple of 8 bytes long ("all"), or only the tap's first body, whose change
    # against the swizzled layout is 84 bytes where the others' is 72 ("q0").  Both measured slower than no padding, on two boxes
    # (profiles/mx_hi_stride_ab.txt): -0.6 ... -0.9 % per launch against the parent where the unpadded bodies give -1.2 %
    if (body_pad == "all" and (mx_body_bytes(L) + 4) % 8) or (body_pad == "q0" and hs == 0):
        L += ["s_nop 0"]
    L += ["s_mov_b32 m0, %[keep]"]
    return mx_ablated(L, ablate, hs)


def emit(name, lines):
    out = ["#define %s \\" % name]
    for l in lines:
        out.append('    "%s\\n\\t" \\' % l)
    out[-1] = out[-1][:-2]
    return "\n".join(out) + "\n"


def write_inc(directory, name, what, text, generator="tools/gen_tower_asm.py"):
    with open(os.path.join(directory, name), "w") as f:
        f.write("// GENERATED by %s — do not edit.  See that script for the issue plan.\n// %s\n%s" % (generator, what, text))


def tower_inc():
    txt = emit("TW8_SLAB_ASM_H0", slab8(0)) + "\n" + emit("TW8_SLAB_ASM_H1", slab8(1))
    txt += "\n// the same with fp16 operands\n"
    txt += emit("TW8F_SLAB_ASM_H0", f16(slab8(0))) + "\n" + emit("TW8F_SLAB_ASM_H1", f16(slab8(1)))
    txt += "\n// slab bodies whose first / second row-tile MFMAs sit behind scalar branches (off-board tiles of a tap), bf16 and fp16\n"
    txt += emit("TW8_SKIPG_ASM_H0", branchy2(slab8(0))) + "\n" + emit("TW8_SKIPG_ASM_H1", branchy2(slab8(1))) + "\n"
    return txt + emit("TW8F_SKIPG_ASM_H0", f16(branchy2(slab8(0)))) + "\n" + emit("TW8F_SKIPG_ASM_H1", f16(branchy2(slab8(1))))


def split_inc():
    txt = ""
    for hs in range(4):
        txt += emit("XS_SLAB_ASM_Q%d" % hs, slabX(hs, XS_LO_OFF)) + "\n" + emit("XSF_SLAB_ASM_Q%d" % hs, f16(slabX(hs, XS_LO_OFF))) + "\n"
    # dy = -1 taps of the strict kernel: the first row tile of cell group 0 (12 padding rows + the 20 rank-0 cells of both positions)
    txt += "// slab bodies whose first-row-tile MFMAs (3 of 9 per k-step) sit behind a scalar branch (dy = -1 taps)\n"
    for hs in range(4):
        b = branchy(slabX(hs, XS_LO_OFF), ("%[c0],",))
        txt += emit("XS_SKIP0_ASM_Q%d" % hs, b) + "\n" + emit("XSF_SKIP0_ASM_Q%d" % hs, f16(b)) + "\n"
    return txt


def mx_inc(**knobs):
    txt = ""
    for hs in range(4):
        txt += emit("MX_SLAB_ASM_Q%d" % hs, slabMX(hs, **knobs)) + "\n"
    txt += "// the same with the first-row-tile MFMAs (3 of 9) behind a scalar branch (dy = -1 taps, cell group 0)\n"
    for hs in range(4):
        txt += emit("MX_SKIP0_ASM_Q%d" % hs, branchy(slabMX(hs, **knobs), ("%[c0],",))) + "\n"
    txt += "// the last slab of a layer: no operand requests, every LDS read of the wave waited for in front of the barrier\n"
    return txt + emit("MX_SLAB_ASM_Q3_LAST", slabMX(3, layer_last=True, **knobs)) + "\n"


def main():
    here = os.path.dirname(os.path.abspath(__file__))
    ap = argparse.ArgumentParser(description="writes cz_tower_slab_asm.inc, cz_trunk_split_asm.inc and cz_trunk_mx_asm.inc")
    ap.add_argument("directory", nargs="?", default=os.path.join(os.path.dirname(here), "cchess_zero_amd", "csrc"))
    ap.add_argument("--ablate", default=(), type=ablate_arg(), help="timing ablations of the mx bodies, comma separated (mx_ablated)")
    ap.add_argument("--dma-place", default="C", choices=("C", "B0", "B0C0", "Cend"))
    ap.add_argument("--body-pad", default="none", choices=("none", "all", "q0"))
    a = ap.parse_args()
    knobs = dict(ablate=a.ablate, dma_place=a.dma_place, body_pad=a.body_pad)
    write_inc(a.directory, "cz_tower_slab_asm.inc", "k_tower8_c128: 8 waves / 4 positions, two fragment sets, 2 DMA pieces per wave and slab", tower_inc())
    write_inc(a.directory, "cz_trunk_split_asm.inc",
              "k_trunk_split_c128: 8 waves / 2 positions, operands split into hi + lo halves, 9 MFMAs per k-step, bf16 and fp16", split_inc())
    write_inc(a.directory, "cz_trunk_mx_asm.inc", "k_trunk_mx_c128: 8 waves / 2 positions, 6 fp16 MFMAs + 3 block-scaled fp6 MFMAs per slab and wave",
              mx_inc(**knobs))
    print("wrote cz_tower_slab_asm.inc (%d instructions per slab), cz_trunk_split_asm.inc (%d), cz_trunk_mx_asm.inc (%d)" %
          (len(slab8(0)), len(slabX(0, XS_LO_OFF)), len(slabMX(1))))


if __name__ == "__main__":
    main()
