"""hip_ops.host_times keeps float64 host copies of device-resident time grids so that a repeated model call does not synchronise.
When the cache is full it forgets old entries, never the one it has just been given: a full clear between the two grids of one
model call (observed_tp, tp_to_predict) made every later call miss on the first of them and synchronise again."""
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("filled", [0, 63, 64, 65, 66, 130])
def test_two_grids_stay_cached_whatever_the_fill(cuda, filled):
    from ode_rl_amd import hip_ops
    hip_ops._t_cache.clear()
    keep = [torch.arange(3, dtype=torch.float64, device=cuda) + k for k in range(filled)]
    for t in keep:
        hip_ops.host_times(t)
    a = torch.arange(3, dtype=torch.float64, device=cuda) / 6
    b = a + 0.5
    want = (a.cpu(), b.cpu())
    hip_ops.host_times(a)
    hip_ops.host_times(b)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = (hip_ops.host_times(a), hip_ops.host_times(b))
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert len(hip_ops._t_cache) <= 66
