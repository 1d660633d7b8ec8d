"""k_trunk_mx_c128's fp16 hi rows on their padded stride (MXGeo::HI_ROWB = 272 bytes, chunks addressed by immediates of the slab
bodies, a 512-byte zero region for the off-board taps): the `dense` and `sparse` exact nets (tests/exactnets.py) at 1 block on
B = 2 rows (one full workgroup) and B = 5 rows (the last workgroup half filled), trunk and head conv outputs equal to the float64
restatement bit for bit.  Helpers and references are tests/test_net_exact.py's (a reference is computed once per net and batch and
shared with that file).

What is NOT repeated here: tests/test_mx_trunk_gpu.py runs B = 1, 3 and 64 rows at 1 and 7 blocks, and tests/test_exactnets_cpu.py
proves on the CPU that the mutation families of exactnets (`wrap`, `tap_dydx`, `cin_swap`, `pos_swap`) change these nets' expected
outputs: a hi-row read of a wrong row (a tap's neighbour, a cell across the board edge, the workgroup's other position) or of a
wrong 16-byte chunk (other input channels) is one of those mutations and cannot give the reference's integers.  The layout itself —
banks, chunk immediates, the zero alias — is walked on the CPU in tests/test_mx_hi_layout_cpu.py.

As in tests/test_mx_trunk_gpu.py the first launch of the session's kernel runs in a child process under its own time limit."""
import os
import subprocess
import sys

import pytest

import exactnets as E
import test_net_exact as X

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_CHILD = """
import sys, torch
sys.path[:0] = [%r, %r]
import exactnets as E
from cchess_zero_amd.net import PolicyValueNet
net = PolicyValueNet(1, "cuda:0", torch.float16, seed=0, split="mx")
assert net.backend == "hip" and net.engine_name == "mx6"
z = net._hip_net_forward(E.planes("dense", 2).cuda())
torch.cuda.synchronize()
assert bool(torch.isfinite(z).all())
print("first launch ok")
""" % (ROOT, os.path.join(ROOT, "tests"))


@pytest.fixture(scope="module")
def first_launch():
    r = subprocess.run([sys.executable, "-c", _CHILD], timeout=150, capture_output=True, text=True)
    assert r.returncode == 0 and "first launch ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])


_CASES = [(f, s) for f, b, seeds in E.CASES["mx6"] if b == 1 and f in ("dense", "sparse") for s in seeds]


@pytest.mark.parametrize("B", [2, 5])
@pytest.mark.parametrize("family,seed", _CASES)
def test_hi_rows_bit_for_bit(first_launch, family, seed, B):
    assert {f for f, _ in _CASES} == {"dense", "sparse"}
    module = X._module(family, 1, seed, E.HALF["mx6"])
    net = X._net(module, "mx6")
    X._compare(net, module, family, 1, seed, "mx6", "dense[:%d]" % B, E.gpu_batches("mx6")["dense"][:B])
