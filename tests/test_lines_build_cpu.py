"""cz_lines.hip compiled to device assembly with the library's flags (no GPU needed): the kernel of cz_search_lines keeps its
two candidate ranks, its two child counts and the line's cursor in registers — no scratch."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_lines_kernel_uses_no_scratch(tmp_path):
    from cchess_zero_amd import build
    assert "cz_lines.hip" in build.SOURCES
    src = os.path.join(ROOT, "cchess_zero_amd", "csrc", "cz_lines.hip")
    out = str(tmp_path / "cz_lines.s")
    flags = [f for f in build.FLAGS if f not in ("-shared", "-fPIC")]
    subprocess.run([build.hipcc()] + flags + ["--offload-device-only", "-S", "-o", out, src], check=True, stdin=subprocess.DEVNULL,
                   stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=600)
    text = open(out).read()
    found = [(m.group(1), int(m.group(2)))
             for m in re.finditer(r"\.name:\s+(\S+)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)", text) if "k_lines" in m.group(1)]
    assert len(found) == 1, found
    assert found[0][1] == 0, "%s uses %d bytes of scratch" % found[0]
