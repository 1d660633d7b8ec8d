"""k_trunk_mx_c128 on the GPU through cz_net_trunk_mx: what a mistake in its slab schedule (ring slots as immediates of the bodies,
operands requested two steps ahead, the ring refilled three slabs ahead, a static wave priority) would break.
tests/test_mx_slab_plan_cpu.py settles the plan on the CPU; here:

  * the first launch of the session's kernel runs in a child process under a time limit of its own (nothing else is launched
    if it does not return);
  * exact-arithmetic nets (tests/exactnets.py, as tests/test_net_exact.py uses them, sharing its references): B = 1, 3 and 64 rows,
    1 and 7 blocks, trunk and head conv outputs equal to the float64 restatement bit for bit — a weight read in front of its
    slab's publication, or of a slot a DMA already overwrites, gives a wrong integer whatever the rounding;
  * what depends on timing needs every CU loaded: one launch of 1024 rows (512 workgroups, two per CU one after the other) gives
    the bits of the same rows evaluated 37 at a time, also under the device-side row count with an odd number of live rows."""
import ctypes as C
import os
import subprocess
import sys

import pytest
import torch

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
z = net._hip_net_forward(E.planes("dense", 3).cuda())
torch.cuda.synchronize()
assert bool(torch.isfinite(z).all())
print("first launch ok")
""" % (ROOT, os.path.join(ROOT, "tests"))


@pytest.fixture(scope="module")
def first_launch():
    r = subprocess.run([sys.executable, "-c", _CHILD], timeout=150, capture_output=True, text=True)
    assert r.returncode == 0 and "first launch ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])


def test_first_launch_returns(first_launch):
    pass


_CASES = [(f, b) for f, b, _ in E.CASES["mx6"] if b in (1, 7)]


@pytest.mark.parametrize("family,blocks", _CASES)
def test_exact_nets_bit_for_bit(first_launch, family, blocks):
    assert {b for _, b in _CASES} == {1, 7}
    seeds = [s for f, b, s in E.CASES["mx6"] if (f, b) == (family, blocks)][0]
    batches = E.gpu_batches("mx6")
    for seed in seeds:
        module = X._module(family, blocks, seed, E.HALF["mx6"])
        net = X._net(module, "mx6")
        for B in (1, 3):
            X._compare(net, module, family, blocks, seed, "mx6", "dense[:%d]" % B, batches["dense"][:B])
        assert batches["live"].shape[0] == 64
        X._compare(net, module, family, blocks, seed, "mx6", "live", batches["live"])


@pytest.fixture(scope="module")
def loaded(first_launch):
    """7 blocks, 1024 distinct rows: one launch each for z + value and for the trunk rows; never modified"""
    from cchess_zero_amd.net import PolicyValueNet
    net = PolicyValueNet(7, "cuda:0", torch.float16, seed=0, split="mx")
    assert net.backend == "hip" and net.engine_name == "mx6"
    x = E.planes("dense", 1024, seed=3).cuda()
    x16 = torch.zeros((1024, 9, 10, 16), dtype=torch.float16, device="cuda")
    x16[..., :14] = x.to(torch.float16)
    z, value = net.search_eval(x16)
    trunk = net._hip_net_forward(x, trunk=True)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(z).all()) and bool(torch.isfinite(value).all()) and bool(torch.isfinite(trunk).all())
    assert float(z.abs().max()) > 0 and int((trunk != 0).sum()) > trunk.numel() // 8
    return net, x, x16, z.clone(), value.clone(), trunk.clone()


def test_1024_rows_equal_the_same_rows_37_at_a_time(loaded):
    net, x, x16, z, value, trunk = loaded
    zs, vs, ts = [], [], []
    for i in range(0, 1024, 37):
        zi, vi = net.search_eval(x16[i:i + 37].contiguous())
        zs.append(zi.clone())
        vs.append(vi.clone())
        ts.append(net._hip_net_forward(x[i:i + 37].contiguous(), trunk=True).clone())
    torch.cuda.synchronize()
    assert torch.equal(torch.cat(zs), z), "z: %d rows differ" % int((torch.cat(zs) != z).any(2).any(1).sum())
    assert torch.equal(torch.cat(vs), value)
    assert torch.equal(torch.cat(ts), trunk), "trunk: %d rows differ" % int((torch.cat(ts) != trunk).any(2).any(1).sum())


def test_1024_rows_under_an_odd_device_row_count(loaded):
    from cchess_zero_amd._lib import check, lib
    net, x, x16, z, value, trunk = loaded
    live = 1001
    n = torch.tensor([live], dtype=torch.int32, device="cuda")
    zc, vc = net.search_eval(x16, C.c_void_p(n.data_ptr()))
    check(lib().cz_set_batch_count(net._hip_ctx().h, C.c_void_p(n.data_ptr())), "cz_set_batch_count")
    try:
        tc = net._hip_net_forward(x, trunk=True)[:live].clone()
    finally:
        check(lib().cz_set_batch_count(net._hip_ctx().h, None), "cz_set_batch_count")
    torch.cuda.synchronize()
    assert torch.equal(zc[:live], z[:live]) and torch.equal(vc[:live], value[:live]) and torch.equal(tc, trunk[:live])
