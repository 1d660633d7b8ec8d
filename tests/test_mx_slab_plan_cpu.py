"""Plan model of k_trunk_mx_c128's slab bodies (no GPU).  The bodies carry their ring slots as immediates (slab g of a layer sits in
slot g & 3 = the body's quarter), request operands two steps ahead under counted waits and refill the ring three slabs ahead under
vmcnt(2): what can go wrong with that is settled here, on the text of the committed bodies
(cchess_zero_amd/csrc/cz_trunk_mx_asm.inc), in the order cz_trunk_mx.h runs them, walked as barrier intervals over three layers:

  1. every body holds exactly one barrier (all eight waves run the same bodies: equal counts);
  2. every weight read of slab s lies behind a barrier at which s is published: every wave has waited (vmcnt) for its own two
     pieces of s in front of that barrier — and the DMA keeps its lead of three slabs;
  3. no DMA targets a ring slot that is still read, or has a read in flight, behind the barrier the DMA follows;
  4. no read of the activation planes is in flight at, or issued behind, the last barrier of a layer (the epilogue overwrites them);
  5. every counted lgkmcnt(N) is exact: N = the reads issued behind the last one the MFMAs up to the next wait consume — and no MFMA
     reads a register with a read in flight;
  6. every ring slot named by a body (weight reads: this slab's or the next slab's; DMA: the slab before's) is the one its quarter
     implies, and the committed bodies are what tools/gen_tower_asm.py plans."""
import importlib.util
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cchess_zero_amd", "csrc")
SLAB, LAYER, LAYERS = 16384, 36, 3


def _gen():
    spec = importlib.util.spec_from_file_location("gen_tower_asm", os.path.join(ROOT, "tools", "gen_tower_asm.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _committed_bodies():
    """macro name -> instruction list, from the committed .inc"""
    bodies, name = {}, None
    for line in open(os.path.join(CSRC, "cz_trunk_mx_asm.inc")):
        m = re.match(r"#define (\w+) \\", line)
        if m:
            name = m.group(1)
            bodies[name] = []
            continue
        m = re.match(r'\s+"(.*)\\n\\t"', line)
        if m and name:
            bodies[name].append(m.group(1))
        elif not line.strip():
            name = None
    return bodies


def _without_skip(body):
    """a dy = -1 body without its scalar branches around the first-row-tile MFMAs (the MFMAs stay): the plain body"""
    assert body[:2] == ["s_cmp_lg_u32 %[skipm], 0", "s_cselect_b64 vcc, -1, 0"]
    assert not any("vcc" in l and l != "s_cbranch_vccnz 1f" for l in body[2:])       # VCC is written once, at the top
    return [l for l in body[2:] if l not in ("s_cbranch_vccnz 1f", "1:")]


def _layer_macros():
    """the bodies of one layer in the kernel's order: 3 taps x SKIP0 Q0-3, 5 taps x SLAB Q0-3, tap 8 = Q0 Q1 Q2 Q3_LAST"""
    src = open(os.path.join(CSRC, "cz_trunk_mx.h")).read()
    runs = re.findall(r"^\s+MX_RUNV?\((\w+),", src, re.M)
    q = ["Q0", "Q1", "Q2", "Q3"]
    assert runs == ["MX_SKIP0_ASM_" + x for x in q] + ["MX_SLAB_ASM_" + x for x in q] + ["MX_SLAB_ASM_Q0", "MX_SLAB_ASM_Q1", "MX_SLAB_ASM_Q2", "MX_SLAB_ASM_Q3_LAST"]
    assert re.search(r"for \(; tap < 3; \+\+tap\)", src) and re.search(r"for \(; tap < 8; \+\+tap\)", src)
    seq = runs[0:4] * 3 + runs[4:8] * 5 + runs[8:12]
    assert len(seq) == LAYER
    return seq


def _regs(tok):
    m = re.match(r"v\[(\d+):(\d+)\]", tok)
    return {"v%d" % i for i in range(int(m.group(1)), int(m.group(2)) + 1)} if m else {tok}


def _sources(ins):
    out = set()
    for t in re.findall(r"%\[\w+\]|v\[\d+:\d+\]", ins.split(" op_sel")[0]):
        if not re.match(r"%\[c\d\]", t):
            out |= _regs(t)
    return out


class Wave:
    """one wave walking the layers; `passed` = barriers passed so far (barrier g is slab g's)"""

    def __init__(self, streams):
        self.streams = streams
        self.passed = 0
        self.lds = []            # reads in flight, oldest first
        self.vm = []             # DMA pieces in flight, oldest first: slab numbers
        self.reads = []          # every weight read: (slab, barriers passed at issue, record)
        self.dmas = []           # (slab, slot, barriers passed at issue)
        self.waited = {}         # slab -> barriers passed when the wave's vmcnt wait covered both of its pieces
        self.barriers_per_body, self.errors, self.last_barrier_clean, self.mfmas = [], [], [], 0

    def err(self, g, msg):
        self.errors.append("slab %d: %s" % (g, msg))

    def run(self):
        for g, body in enumerate(self.streams):
            hs, last = g % 4, g % LAYER == LAYER - 1
            if g % LAYER == 0:      # the C++ preload of the layer's first two operand sets: plain reads of slab g, waited for by the compiler
                for _ in range(2):
                    self.reads.append((g, self.passed, {"slab": g, "done": self.passed, "dst": set(), "act": False}))
            m0, nbar = None, 0
            for k, ins in enumerate(body):
                op = ins.split()[0]
                if op == "s_waitcnt":
                    v, l = re.search(r"vmcnt\((\d+)\)", ins), re.search(r"lgkmcnt\((\d+)\)", ins)
                    if v:
                        while len(self.vm) > int(v.group(1)):
                            s = self.vm.pop(0)
                            if s not in self.vm:
                                self.waited[s] = self.passed
                    if l:
                        n = int(l.group(1))
                        if not (n == 0 and body[k + 1] == "s_barrier"):      # (the layer's last barrier drains everything: item 4)
                            need = set()
                            for nxt in body[k + 1:]:
                                if nxt.startswith("s_waitcnt") and "lgkmcnt" in nxt:
                                    break
                                if nxt.startswith("v_mfma"):
                                    need |= _sources(nxt)
                            idx = [i for i, r in enumerate(self.lds) if r["dst"] & need]
                            if idx and len(self.lds) - 1 - idx[-1] != n:
                                self.err(g, "%s but %d reads were issued behind the last one its MFMAs consume" % (ins, len(self.lds) - 1 - idx[-1]))
                        while len(self.lds) > n:
                            self.lds.pop(0)["done"] = self.passed
                elif op == "s_barrier":
                    if last:
                        self.last_barrier_clean.append(not any(r["act"] for r in self.lds))
                    self.passed += 1
                    nbar += 1
                elif op.startswith("ds_read"):
                    m = re.match(r"ds_read_b\d+ (\S+), %\[(\w+)\](?: offset:(\d+))?", ins)
                    base, off = m.group(2), int(m.group(3) or 0)
                    rec = {"dst": _regs(m.group(1)), "done": None, "act": base not in ("vb", "vy", "vs")}
                    if not rec["act"]:
                        slot = off // SLAB
                        if slot not in (hs, (hs + 1) % 4):
                            self.err(g, "weight read of ring slot %d in a body of quarter %d: %s" % (slot, hs, ins))
                        rec["slab"] = g if slot == hs else g + 1
                        self.reads.append((rec["slab"], self.passed, rec))
                    elif last and nbar:
                        self.err(g, "activation read behind the layer's last barrier: " + ins)
                    self.lds.append(rec)
                elif op == "s_add_u32" and ins.split()[1] == "m0,":
                    m0 = int(ins.split()[-1], 16)
                elif op == "s_mov_b32" and ins.split()[1] == "m0,":
                    m0 = None
                elif op.startswith("global_load_lds"):
                    if m0 // SLAB != (hs + 3) % 4 or m0 % SLAB not in (0, 0x2000):
                        self.err(g, "DMA to ring offset 0x%x in a body of quarter %d" % (m0, hs))
                    self.dmas.append((g + 3, m0 // SLAB, self.passed))
                    self.vm.append(g + 3)
                elif op.startswith("v_mfma"):
                    if any(r["dst"] & _sources(ins) for r in self.lds):
                        self.err(g, "MFMA reads a register with a read in flight: " + ins)
                    self.mfmas += 1
            self.barriers_per_body.append(nbar)
        return self


@pytest.fixture(scope="module")
def walk():
    gen, bodies, seq = _gen(), _committed_bodies(), _layer_macros()
    plain = {n: (_without_skip(b) if "SKIP0" in n else b) for n, b in bodies.items()}
    return gen, bodies, plain, seq, Wave([plain[n] for n in seq] * LAYERS).run()


def test_committed_bodies_are_the_generators_plan(walk):
    gen, bodies, plain, seq, _ = walk
    for name in sorted(set(seq)):
        assert plain[name] == gen.slabMX(int(name.split("_Q")[1][0]), name.endswith("_LAST")), name
    for hs in range(4):     # a dy = -1 body is the plain body with three MFMAs behind branches
        skip = bodies["MX_SKIP0_ASM_Q%d" % hs]
        assert skip.count("s_cbranch_vccnz 1f") == 3 and all(skip[i + 1].split()[1] == "%[c0]," and skip[i + 2] == "1:" for i, l in enumerate(skip) if l == "s_cbranch_vccnz 1f")


def test_one_barrier_per_body(walk):
    """item 1"""
    w = walk[4]
    assert w.barriers_per_body == [1] * (LAYER * LAYERS) and w.mfmas == 9 * LAYER * LAYERS


def test_counted_waits_and_slot_immediates_are_exact(walk):
    """items 5 and 6"""
    w = walk[4]
    assert not w.errors, "\n".join(w.errors[:10])


def test_weight_reads_lie_behind_their_slabs_publication(walk):
    """item 2.  Slab s is published by the first barrier in front of which every wave (they all run these bodies) has waited for its
    own pieces of s; slabs 0-2 land in the prologue, in front of a __syncthreads"""
    w = walk[4]
    pub = lambda s: -1 if s < 3 else w.waited.get(s, 10 ** 9)
    for slab, passed, _ in w.reads:
        assert pub(slab) <= passed - 1, "slab %d is read behind %d barriers, published by barrier %d" % (slab, passed, pub(slab))
    assert all(w.waited[s] == s - 1 for s in range(3, LAYER * LAYERS))      # waited for no earlier than in front of barrier s - 1


def test_no_dma_into_a_slot_that_is_still_read(walk):
    """item 3: the DMA of slab s + 4 into the slot of slab s follows a barrier; every read of slab s has been waited for in front of it"""
    w = walk[4]
    for slab, slot, passed in w.dmas:
        assert slot == slab % 4
        recs = [rec for s, _, rec in w.reads if s == slab - 4]
        assert slab < 4 or len(recs) == 5      # w0, w1, the fp6 block's two parts, its scales
        for rec in recs:
            assert rec["done"] is not None and rec["done"] <= passed - 1, (slab, rec)


def test_activation_planes_are_quiet_at_a_layers_last_barrier(walk):
    """item 4"""
    assert walk[4].last_barrier_clean == [True] * LAYERS
