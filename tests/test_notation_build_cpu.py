"""cz_notation.hip compiled to device assembly with the library's flags (no GPU needed): the token replay decodes from the lane's
LDS row and never indexes the 23 board words at run time — no scratch at either rule level —, its LDS (the replay's, plus the
staged srcdst table) still lets three waves share a CU, cz_games.hip still yields exactly its two kernels, and the entry point
is bound."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
META = r"\.name:\s+(\S+)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)"


def _asm(tmp_path, name):
    from cchess_zero_amd import build
    assert name in build.SOURCES
    out = str(tmp_path / (name + ".s"))
    flags = [f for f in build.FLAGS if f not in ("-shared", "-fPIC")]
    subprocess.run([build.hipcc()] + flags + ["--offload-device-only", "-S", "-o", out, os.path.join(ROOT, "cchess_zero_amd", "csrc", name)], check=True,
                   stdin=subprocess.DEVNULL, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=600)
    return open(out).read()


def test_read_kernels_use_no_scratch_and_three_waves_share_a_cu(tmp_path):
    text = _asm(tmp_path, "cz_notation.hip")
    found = [(m.group(1), int(m.group(2))) for m in re.finditer(META, text) if "k_games_read" in m.group(1)]
    assert len(found) == 2, found          # rules 0 and rules 1
    for name, scratch in found:
        assert scratch == 0, "%s uses %d bytes of scratch" % (name, scratch)
    assert not [m.group(1) for m in re.finditer(META, text) if "k_games_replay" in m.group(1)]
    lds = [int(x) for x in re.findall(r"\.group_segment_fixed_size:\s+(\d+)", text)]
    assert len(lds) == 2 and max(lds) * 3 <= 160 * 1024, lds


def test_the_replay_source_still_yields_its_two_kernels(tmp_path):
    text = _asm(tmp_path, "cz_games.hip")
    names = [m.group(1) for m in re.finditer(META, text)]
    assert len(names) == 2 and all("k_games_replay" in n for n in names), names


def test_the_entry_point_is_bound():
    from cchess_zero_amd import _lib
    assert "cz_games_read" in _lib.EXPORTS and len(_lib._SIGS["cz_games_read"][1]) == 18
    assert _lib.GAME_AMBIGUOUS == 5 and _lib.GAME_STATUS[5] == "ambiguous"
    L = _lib.lib()                       # a NULL context is refused before anything else is touched (no GPU needed)
    assert L.cz_games_read(*([None] * 4 + [0, None, None, 0, 0, None, 0] + [None] * 7)) < 0 and b"cz_games_read" in L.cz_last_error()
    header = open(os.path.join(ROOT, "include", "cchess_hip.h")).read()
    assert re.search(r"#define CZ_GAME_AMBIGUOUS 5\b", header) and "int cz_games_read(cz_ctx *" in header
