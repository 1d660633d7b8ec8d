"""k_trunk_mx_c128's fp16 hi rows (no GPU): rows on a padded stride of MXGeo::HI_ROWB = 272 bytes, 16-byte chunk c of a row at 16 c,
the chunk an immediate of the slab bodies, and a 512-byte zero region that off-board taps read at 16 (row & 15) + the same immediate.
Walked here from the header's constants (cchess_zero_amd/csrc/cz_trunk_mx.h), the committed bodies (cz_trunk_mx_asm.inc) and the
generator's plan (tools/gen_tower_asm.py), under the LDS model of gfx950: a ds_read_b128 is served in four groups of sixteen lanes,
{0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} and the same of lanes 32-63, bank = (address / 4) mod 64, four banks per lane; a
ds_write_b64 in four groups of sixteen consecutive lanes, bank = (address / 4) mod 32, two banks per lane; within a group two
DIFFERENT addresses on one bank cost a cycle, equal addresses broadcast.

  1. reads: 6 row tiles (2 cell groups x 3) x 9 taps x the 8 chunk immediates of the bodies x both k-halves, the twelve padding
     lanes and the off-board lanes included, with the kernel's row of a lane (32 tile + lane - 12; row = 20 y + 10 p + x): no group
     has two addresses on one bank; an on-board lane reads chunk c + k-half of its tap's row; a masked lane reads inside the zero region;
  2. stores: the epilogue's ds_write_b64 of the hi rows cost no more conflict cycles than the 256-byte rows with the XOR swizzle did;
  3. the bodies' immediates are 16 x the chunks the generator plans for their quarter (the NEXT slab's 32 input channels; the fourth
     body of a tap reads at the next tap's addresses), and no body holds a VALU instruction besides its MFMAs;
  4. LDS_TOTAL fits the CU's 160 KB, and the header states the layout's invariants."""
import importlib.util
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cchess_zero_amd", "csrc")
READ_GROUPS = [[0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27], [4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31]]
READ_GROUPS = READ_GROUPS + [[l + 32 for l in g] for g in READ_GROUPS]
WRITE_GROUPS = [list(range(16 * g, 16 * g + 16)) for g in range(4)]


def _gen():
    spec = importlib.util.spec_from_file_location("gen_tower_asm", os.path.join(ROOT, "tools", "gen_tower_asm.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@pytest.fixture(scope="module")
def header():
    return open(os.path.join(CSRC, "cz_trunk_mx.h")).read()


@pytest.fixture(scope="module")
def geo(header):
    """MXGeo's constants, evaluated from the header's own expressions"""
    env = {}
    for name in ("CV_ROWB", "TW_NBUF"):
        env[name] = int(re.search(r"constexpr int %s = (\d+);" % name, open(os.path.join(CSRC, "cz_conv_kernel.h")).read()).group(1))
    body = re.search(r"struct MXGeo \{(.*?)\n\};", header, re.S).group(1)
    for decl in re.findall(r"static constexpr int ([^;]+);", body):
        for part in decl.split(","):
            name, expr = part.split("=")
            env[name.strip()] = eval(expr.replace("/", "//"), {}, env)
    return env


@pytest.fixture(scope="module")
def bodies():
    out, name = {}, None
    for line in open(os.path.join(CSRC, "cz_trunk_mx_asm.inc")):
        m = re.match(r"#define (\w+) \\", line)
        if m:
            name = m.group(1)
            out[name] = []
            continue
        m = re.match(r'\s+"(.*)\\n\\t"', line)
        if m and name:
            out[name].append(m.group(1))
        elif not line.strip():
            name = None
    assert len(out) == 9
    return out


def _hi_reads(body):
    """(operand set, tile, base operand, immediate) of a body's hi-row reads"""
    return [(int(m.group(1)), int(m.group(2)), m.group(3), int(m.group(5)))
            for m in (re.match(r"ds_read_b128 %\[a(\d)h(\d)\], %\[(n?ab)(\d)\] offset:(\d+)$", l) for l in body) if m]


def _lane_rows(wr, i):
    """the kernel's rowk of lanes 0..31 of row tile i of cell group wr (negative: the twelve padding lanes)"""
    return [32 * (wr * 3 + i) + l - 12 for l in range(32)]


def _tap_base(geo, k, tap, khalf):
    """tap_addr: (ab of a lane whose own row is k, on board?, the row it reads or would have read)"""
    kk0 = max(k, 0)
    h, rem = divmod(kk0, 20)
    p, w = divmod(rem, 10)
    assert kk0 == 20 * h + 10 * p + w
    y, x = h + tap // 3 - 1, w + tap % 3 - 1
    on = k >= 0 and 0 <= y < 9 and 0 <= x < 10
    kk = k + (tap // 3 - 1) * 20 + (tap % 3 - 1)
    if on:
        assert kk == 20 * y + 10 * p + x and 0 <= kk < geo["ROWS"]
    ab = (geo["HI_OFF"] + kk * geo["HI_ROWB"] if on else geo["ZERO_OFF"] + ((kk & 15) << 4)) + (khalf << 4)
    return ab, on, kk


def _conflict_cycles(addrs, width, nbanks):
    """extra LDS cycles of one lane group: addrs = the lanes' byte addresses (None: lane masked off by EXEC)"""
    per_bank = {}
    for a in addrs:
        if a is not None:
            for d in range(width // 4):
                per_bank.setdefault((a // 4 + d) % nbanks, set()).add(a)
    return max([len(s) for s in per_bank.values()] + [1]) - 1


def test_header_states_the_layout(header, geo):
    assert geo["HI_ROWB"] == 272 and geo["HI_ROWB"] % 16 == 0 and (geo["HI_ROWB"] // 4) % 64 == 4
    assert geo["HI_OFF"] % 16 == 0 and geo["W_OFF"] % 16 == 0
    assert geo["ZERO_OFF"] % 256 == geo["HI_OFF"] % 256 and geo["ZERO_BYTES"] == 512
    assert geo["HI_OFF"] + geo["ROWS"] * geo["HI_ROWB"] <= geo["ZERO_OFF"] and geo["ZERO_OFF"] + geo["ZERO_BYTES"] <= geo["W_OFF"]
    assert geo["ROWS"] * geo["F32_ROWB"] <= geo["HEADW_OFF"]
    assert geo["LDS_TOTAL"] == geo["HEADW_OFF"] + 3 * 128 * 4 and geo["LDS_TOTAL"] <= 163840
    # the C++ around the bodies computes what this file walks
    assert "ab[i] = (on ? Geo::HI_OFF + kk * Geo::HI_ROWB : Geo::ZERO_OFF + ((kk & 15) << 4)) + (khalf << 4);" in header
    assert "const int k = 32 * (wr * 3 + i) + l31 - 12;" in header and "const int kk = rowk[i] + delta;" in header
    assert "const int rowb = Geo::HI_OFF + rkk[i] * Geo::HI_ROWB;" in header and "smem + rowb + (n0 << 1)" in header
    assert "if (tid < Geo::ZERO_BYTES / 16) *reinterpret_cast<uint4 *>(smem + Geo::ZERO_OFF + (tid << 4))" in header
    for needle in ("HI_ROWB % 16 == 0", "(MXGeo::HI_ROWB / 4) % 64 == 4", "(MXGeo::ZERO_OFF - MXGeo::HI_OFF) % 256 == 0",
                   "MXGeo::ROWS * MXGeo::F32_ROWB <= MXGeo::HEADW_OFF", "MXGeo::LDS_TOTAL <= 163840"):
        assert needle in header[header.index("};"):header.index("typedef unsigned u32x6")], needle
    assert "lds_addr" not in header and "key" not in re.sub(r"//.*", "", header)      # nothing swizzles the hi rows any more


def test_immediates_are_the_planned_chunks_and_no_valu_is_left(bodies):
    gen = _gen()
    seen = set()
    for name, body in bodies.items():
        hs, reads = int(name.split("_Q")[1][0]), _hi_reads(body)
        assert not [l for l in body if l.startswith("v_") and not l.startswith("v_mfma")], name
        assert not [l for l in body if re.search(r"%\[(n?key\d|t\d)\]", l)], name
        if name.endswith("_LAST"):
            assert not reads
            continue
        # body hs requests the next slab's operands: input channels 32 (hs + 1) .. of the tap = chunks 4 (hs + 1), + 2 of a row (8 fp16
        # per chunk, the upper k-half one chunk on); behind the tap's fourth slab the next tap's chunks 0 and 2
        ca, cb = ((hs + 1) % 4) * 4, ((hs + 1) % 4) * 4 + 2
        assert gen.mx_hi_chunks(hs) == (ca, cb)
        assert sorted(reads) == sorted([(0, i, "nab" if hs == 3 else "ab", 16 * ca) for i in range(3)] +
                                       [(1, i, "nab" if hs == 3 else "ab", 16 * cb) for i in range(3)]), name
        seen |= {imm for _, _, _, imm in reads}
    assert seen == {16 * c for c in range(0, 16, 2)}


def test_hi_row_reads_are_conflict_free_and_land_where_they_should(geo, bodies, header):
    imms = sorted({imm for b in bodies.values() for _, _, _, imm in _hi_reads(b)})
    assert len(imms) == 8
    # the layer's preload reads chunks 0 and 2 through the same bases
    assert "smem + ab[i]);" in header and "smem + ab[i] + (2 << 4));" in header and {0, 32} <= set(imms)
    masked = on_board = 0
    for wr in range(2):
        for i in range(3):
            rows = _lane_rows(wr, i)
            for tap in range(9):
                for imm in imms:
                    addr = {}
                    for khalf in range(2):
                        for l31, k in enumerate(rows):
                            ab, on, kk = _tap_base(geo, k, tap, khalf)
                            a = ab + imm
                            addr[32 * khalf + l31] = a
                            assert a % 16 == 0
                            if on:
                                assert a == geo["HI_OFF"] + kk * geo["HI_ROWB"] + 16 * (imm // 16 + khalf) and imm // 16 + khalf < 16
                                on_board += 1
                            else:
                                assert geo["ZERO_OFF"] <= a and a + 16 <= geo["ZERO_OFF"] + geo["ZERO_BYTES"]
                                # the banks of the row it would have read
                                assert (a // 4) % 64 == ((geo["HI_OFF"] + kk * geo["HI_ROWB"] + imm + 16 * khalf) // 4) % 64
                                masked += 1
                    for g in READ_GROUPS:
                        assert _conflict_cycles([addr[l] for l in g], 16, 64) == 0, (wr, i, tap, imm, g)
    assert on_board + masked == 6 * 9 * 8 * 64 and masked >= 12 * 9 * 8 * 2      # (the padding lanes are masked for every tap)


def test_hi_row_stores_cost_no_more_conflicts_than_the_swizzled_rows(geo):
    """store_tile: lane (l31, khalf) of wave (wr, ct) writes 8 bytes = channels n0 .. n0 + 3, n0 = 32 ct + 8 q + 4 khalf, of its row;
    the padding lanes are switched off.  parent: 256-byte rows from HI_OFF, chunk n0 / 8 at (n0 / 8) ^ (absolute 256-byte row & 15)"""
    def parent(r, n0):
        rowb = geo["HI_OFF"] + r * 256
        return rowb + (((n0 >> 3) ^ ((rowb >> 8) & 15)) << 4) + ((n0 & 4) << 1)

    def new(r, n0):
        return geo["HI_OFF"] + r * geo["HI_ROWB"] + 2 * n0

    cost = {"parent": 0, "new": 0}
    for wr in range(2):
        for ct in range(4):
            for i in range(3):
                rows = _lane_rows(wr, i)
                for q in range(4):
                    for name, f in (("parent", parent), ("new", new)):
                        addr = [f(rows[l & 31], 32 * ct + 8 * q + 4 * (l >> 5)) if rows[l & 31] >= 0 else None for l in range(64)]
                        live = [a for a in addr if a is not None]
                        assert len(set(live)) == len(live) and all(a % 8 == 0 for a in live)
                        if name == "new":      # inside the row, clear of the padding and of the next row
                            assert all(0 <= (a - geo["HI_OFF"]) % geo["HI_ROWB"] <= 248 and a + 8 <= geo["ZERO_OFF"] for a in live)
                        cost[name] += sum(_conflict_cycles([addr[l] for l in g], 8, 32) for g in WRITE_GROUPS)
    print("hi-row store conflict cycles per workgroup and layer: parent %d, padded %d" % (cost["parent"], cost["new"]))
    assert cost["new"] <= cost["parent"]
