"""cz_games.hip compiled to device assembly with the library's flags (no GPU needed): the replay kernel keeps a game's board as
23 words in registers across all plies and never indexes them at run time — no scratch at either rule level."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_replay_kernel_uses_no_scratch(tmp_path):
    from cchess_zero_amd import build
    assert "cz_games.hip" in build.SOURCES
    src = os.path.join(ROOT, "cchess_zero_amd", "csrc", "cz_games.hip")
    out = str(tmp_path / "cz_games.s")
    flags = [f for f in build.FLAGS if f not in ("-shared", "-fPIC")]
    subprocess.run([build.hipcc()] + flags + ["--offload-device-only", "-S", "-o", out, src], check=True, stdin=subprocess.DEVNULL,
                   stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=600)
    text = open(out).read()
    found = [(m.group(1), int(m.group(2)))
             for m in re.finditer(r"\.name:\s+(\S+)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)", text) if "k_games_replay" in m.group(1)]
    assert len(found) == 2, found          # rules 0 and rules 1
    for name, scratch in found:
        assert scratch == 0, "%s uses %d bytes of scratch" % (name, scratch)
    # three waves per CU need the wave's LDS below a third of the CU's 160 KB
    lds = [int(x) for x in re.findall(r"\.group_segment_fixed_size:\s+(\d+)", text)]
    assert lds and max(lds) * 3 <= 160 * 1024, lds


def test_the_entry_point_is_bound():
    from cchess_zero_amd import _lib
    assert "cz_games_replay" in _lib.EXPORTS and len(_lib._SIGS["cz_games_replay"][1]) == 17
