"""Exact-global step control installed with odehip_set_norm_allreduce_counted turns no adaptive method away: a bosh3 call gets as far
as a dopri5 call does (under odehip_set_norm_allreduce it stays refused: tests/test_adaptive_abi_cpu.py).  Checkable without a device, because the arguments are looked at before any HIP call: a descriptor without
weights is the first thing either method trips over, and the callback is never reached.  (On the GPU: tests/test_hip_bosh3_global_control.py.)"""
import ctypes

EINVAL = -1


def test_bosh3_under_the_counted_hook_is_not_refused():
    from ode_rl_amd import _lib as L
    lib, d = L.load(), L.ConvStack()
    d.n_convs, d.ks = 3, 3
    for i in range(4):
        d.channels[i] = 64
    called = []
    cb = L.ALLREDUCE_FN(lambda ptr, n, stream, user: called.append(n) or 1)
    p = ctypes.c_void_p(256)   # never dereferenced
    t = (ctypes.c_double * 2)(0.0, 1.0)
    assert lib.odehip_set_norm_allreduce_counted(ctypes.cast(cb, ctypes.c_void_p), None, 2, p) == 0
    try:
        msgs = {}
        for code in (L.BOSH3, L.DOPRI5):
            rc = lib.odehip_odeint_adaptive(code, ctypes.byref(d), p, t, 2, 1, 1e-3, 1e-4, 0.0, 0, 0, p, None, None, 0, p, 1 << 40, None)
            assert rc == EINVAL
            msgs[code] = lib.odehip_last_error()
        assert b"not implemented" not in msgs[L.BOSH3] and b"null weights" in msgs[L.BOSH3], msgs
        assert msgs[L.BOSH3] == msgs[L.DOPRI5]
        assert not called
        # installing with the older call afterwards puts its contract back: dopri5 only
        assert lib.odehip_set_norm_allreduce(ctypes.cast(cb, ctypes.c_void_p), None, 2, p) == 0
        rc = lib.odehip_odeint_adaptive(L.BOSH3, ctypes.byref(d), p, t, 2, 1, 1e-3, 1e-4, 0.0, 0, 0, p, None, None, 0, p, 1 << 40, None)
        assert rc == EINVAL and b"is not implemented for bosh3" in lib.odehip_last_error()
    finally:
        assert lib.odehip_set_norm_allreduce(None, None, 1, None) == 0
