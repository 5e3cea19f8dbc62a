"""Thin torch-facing wrappers over the C ABI: pointer plumbing, workspace and packed-weight caches.

Nothing here computes: every function hands raw device pointers to libodecgru_hip.so on torch's
current stream.  Tensors must be CUDA fp32; anything else raises (there is no CPU fallback).
"""
import ctypes
import os
import threading
import weakref

import numpy as np
import torch

from . import _lib

_workspaces = {}


_last_stream = None   # the stream the library's process-global state (workspace caches, flag areas, layer tables) was last used on


def _stream():
    """The caller's current stream, handed to the C ABI.  The library's state is process-global (ONE
    process per GPU, one stream at a time): calls on a second DEVICE are refused, and when the current stream CHANGES the new
    stream first waits for everything enqueued on the previous one, so two streams can never run library launches that share a
    workspace or flag area concurrently.  (Under graph capture the wait cannot be expressed -- an event from outside the capture
    -- and the capturing caller has ordered its streams itself.)"""
    global _last_stream
    cur = torch.cuda.current_stream()
    if _last_stream is None:
        _last_stream = cur
    elif cur != _last_stream:
        if cur.device != _last_stream.device:
            raise RuntimeError(f"ode_rl_amd drives ONE GPU per process: first used on {_last_stream.device}, now called on {cur.device}")
        if not torch.cuda.is_current_stream_capturing():
            cur.wait_stream(_last_stream)
        _last_stream = cur
    return ctypes.c_void_p(cur.cuda_stream)


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def require_device_tensor(t, name):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor")
    if not t.is_cuda:
        raise RuntimeError(f"{name} is on {t.device}: the HIP path needs CUDA (ROCm) tensors and has no CPU fallback")
    if t.dtype != torch.float32:
        raise TypeError(f"{name} must be float32 (got {t.dtype})")


_CANARY = 4096          # guard bytes behind every workspace: a kernel that overruns its carve-out trips check_canaries()
_guarded = []           # weak references to (full buffer, payload bytes)


def alloc_workspace(nbytes, device):
    """A fresh workspace of `nbytes` with a guard region behind it; returns the payload view (numel() == nbytes)."""
    nbytes = max(int(nbytes), 1024)
    full = torch.empty(nbytes + _CANARY, dtype=torch.uint8, device=device)
    full[nbytes:].fill_(0xA5)
    view = full[:nbytes]
    if len(_guarded) >= 64:   # forget workspaces that have been freed (one is allocated per training-mode forward)
        _guarded[:] = [(r, n) for r, n in _guarded if r() is not None]
    _guarded.append((weakref.ref(full), nbytes))
    view._odehip_full = full   # keeps the guard alive as long as the view
    return view


def check_canaries():
    """Raises if any live workspace's guard bytes were overwritten (tests call this after every GPU test)."""
    alive = []
    for ref, nbytes in _guarded:
        full = ref()
        if full is None:
            continue
        alive.append((ref, nbytes))
        if not bool((full[nbytes:] == 0xA5).all()):
            raise RuntimeError(f"a HIP kernel wrote beyond its {nbytes}-byte workspace")
    _guarded[:] = alive


def workspace(key, nbytes, device):
    """Persistent per-shape scratch so that pointers stay stable across calls (graph replay)."""
    k = (key, device)
    buf = _workspaces.get(k)
    if buf is None or buf.numel() < nbytes:
        buf = alloc_workspace(nbytes, device)
        _workspaces[k] = buf
    return buf


_t_cache = {}


def host_times(t):
    """float64 host copy of a 1-D time tensor.  A device-resident `t` costs a device->host copy (a stream synchronisation);
    it is cached per (base tensor OBJECT, version, view geometry): the base is held by weak reference, so a new tensor that
    happens to reuse the address of a freed one can never hit the cache."""
    if not isinstance(t, torch.Tensor):
        t = torch.as_tensor(t, dtype=torch.float64)
    if t.dim() != 1:
        raise AssertionError("`t` must be one dimensional")
    if not t.is_cuda:
        return t.detach().to(torch.float64)
    base = t._base if t._base is not None else t
    key = (id(base), base._version, t.storage_offset(), t.numel(), t.stride(0) if t.numel() > 1 else 1, t.dtype)
    hit = _t_cache.get(key)
    if hit is not None and hit[0]() is base:
        return hit[1]
    if len(_t_cache) > 64:   # forget the tensors that are gone, then the oldest entries -- never the whole cache: clearing it between
        for k in [k for k, v in _t_cache.items() if v[0]() is None]:   # the two time grids of one model call made every later call
            del _t_cache[k]                                             # miss on the first of them
        for k in list(_t_cache)[:max(len(_t_cache) - 32, 0)]:
            del _t_cache[k]
    host = t.detach().to("cpu", torch.float64)
    _t_cache[key] = (weakref.ref(base), host)
    return host


def nchw_to_q4(x):
    require_device_tensor(x, "x")
    x = x.contiguous()
    b, c, h, w = x.shape
    if (h, w) != (16, 16):
        raise ValueError(f"latent maps must be 16x16 (got {h}x{w})")
    out = torch.empty((b, c // 4, 256, 4), dtype=torch.float32, device=x.device)
    _lib.check(_lib.load().odehip_nchw_to_q4(_ptr(x), _ptr(out), b, c, _stream()))
    return out


def q4_to_nchw(x):
    require_device_tensor(x, "x")
    b, q = x.shape[0], x.shape[1]
    out = torch.empty((b, q * 4, 16, 16), dtype=torch.float32, device=x.device)
    _lib.check(_lib.load().odehip_q4_to_nchw(_ptr(x), _ptr(out), b, q * 4, _stream()))
    return out


def _pack_single(entry, w, transpose_flip, dtype, ks=None, per_pair=None, ks_error=None):
    """One conv weight through one packing entry point.  ks: the kernel size the entry point is built for (None: any, and the entry
    point is told the size); per_pair: values of the image per (cout, cin) pair (None: k * k); ks_error: the text raised for a
    non-square kernel or one of another size than ks (None: not checked)."""
    require_device_tensor(w, "weight")
    w = w.detach().contiguous()
    co, ci, k, k2 = w.shape
    if ks_error is not None and (k != k2 or ks not in (None, k)):
        raise ValueError(ks_error)
    if transpose_flip:
        co, ci = ci, co
    out = torch.empty(co * ci * (per_pair or k * k2), dtype=dtype, device=w.device)
    size = () if ks else (k,)   # an entry point built for one kernel size takes no size argument
    _lib.check(getattr(_lib.load(), entry)(_ptr(w), _ptr(out), co, ci, *size, int(bool(transpose_flip)), _stream()))
    return out


def pack_conv_weight(w, transpose_flip=False):
    """(Cout,Cin,k,k) fp32 -> MFMA-ordered image.  With transpose_flip the result is the packed weight of
    the input-gradient conv (Cin and Cout swap roles)."""
    return _pack_single("odehip_pack_conv_weight", w, transpose_flip, torch.float32, ks_error="square kernels only")


def pack_conv_weight_winograd(w, transpose_flip=False):
    """(Cout,Cin,3,3) fp32 -> Winograd F(2x2,3x3) image U = G g G^T (16 values per channel pair)."""
    return _pack_single("odehip_pack_conv_weight_winograd", w, transpose_flip, torch.float32, ks=3, per_pair=16,
                        ks_error="Winograd form exists for 3x3 kernels only")


def pack_conv_weights_many(jobs):
    """jobs: [(weight (cout,cin,k,k), kind, transpose_flip: bool)], kind 0 / False = pack_conv_weight, 1 / True =
    pack_conv_weight_winograd (3x3), 2 = pack_conv_weight_winograd5 (5x5) -> list of packed tensors, identical to those calls' results
    but ONE launch per 32 jobs (odehip_pack_conv_weights)."""
    outs, recs = [], []
    for w, kind, tf in jobs:
        kind = int(kind)
        require_device_tensor(w, "conv weight")
        w = w.detach().contiguous()
        co, ci, k, _ = w.shape
        if tf:
            co, ci = ci, co
        out = torch.empty(co * ci * (16 if kind == 1 else (36 if kind == 2 else k * k)), dtype=torch.float32, device=w.device)
        outs.append(out)
        recs.append((w, out, co, ci, k, kind, 1 if tf else 0))
    lib = _lib.load()
    for i in range(0, len(recs), _lib.MAX_PACK_JOBS):
        chunk = recs[i:i + _lib.MAX_PACK_JOBS]
        arr = (_lib.PackJob * len(chunk))()
        for j, (w, out, co, ci, k, kind, tf) in enumerate(chunk):
            arr[j].w, arr[j].out, arr[j].cout, arr[j].cin, arr[j].ks, arr[j].kind, arr[j].transpose_flip = _ptr(w), _ptr(out), co, ci, k, kind, tf
        _lib.check(lib.odehip_pack_conv_weights(ctypes.cast(arr, ctypes.c_void_p), len(chunk), _stream()))
    return outs


def pack_conv_weight_winograd5(w, transpose_flip=False):
    """(Cout,Cin,5,5) fp32 -> Winograd F(2x2,5x5) image U = G g G^T (36 values per channel pair; csrc/conv_wino5.hip)."""
    return _pack_single("odehip_pack_conv_weight_winograd5", w, transpose_flip, torch.float32, ks=5, per_pair=36,
                        ks_error="this Winograd form is for 5x5 kernels")


def winograd5_enabled():
    """F(2x2,5x5) for the ConvGRU's fp32 5x5 convolutions: on by default, ODEHIP_WINO5=0 runs the direct kernel (A/B, tests)."""
    return os.environ.get("ODEHIP_WINO5", "1") != "0"


# ---- compute dtype of the 3x3 conv layers: "f32" (exact fp32 MFMA, default) or "bf16" (bf16 operands, fp32 accumulation;
# state, stage combines and conv outputs stay fp32).  bf16 is chosen by set_compute_dtype("bf16") or, as the reference's
# users would ask for it, by running under torch.autocast(device_type="cuda", dtype=torch.bfloat16).
_global_mode = None
_forced = threading.local()


def set_compute_dtype(mode):
    """"f32", "bf16", or None (= follow torch.autocast)."""
    global _global_mode
    if mode not in (None, "f32", "bf16"):
        raise ValueError('compute dtype must be "f32", "bf16" or None')
    _global_mode = mode


# Tanh hidden layers in bf16 mode are opt-in: what a Tanh stack did there before -- TypeError at dispatch -- stays the default, and
# the derivative they get is a rule of this mode (1 - bf16(y)^2 with y the Tanh output as the next conv consumed it), not what
# autograd forms from the fp32 y.
_bf16_tanh = False


def set_bf16_tanh(enabled):
    """Let stacks with Tanh hidden layers (no Tanh head) run in bf16 compute mode; returns the previous setting."""
    global _bf16_tanh
    was, _bf16_tanh = _bf16_tanh, bool(enabled)
    return was


def current_compute_dtype():
    forced = getattr(_forced, "mode", None)
    if forced is not None:
        return forced
    if _global_mode is not None:
        return _global_mode
    try:
        on, dt = torch.is_autocast_enabled("cuda"), torch.get_autocast_dtype("cuda")
    except TypeError:   # older signatures
        on, dt = torch.is_autocast_enabled(), torch.get_autocast_gpu_dtype()
    return "bf16" if (on and dt == torch.bfloat16) else "f32"


class compute_mode:
    """Pins the compute dtype inside a backward pass to the one its forward ran with (autocast is not active on the autograd
    engine's thread)."""

    def __init__(self, mode):
        self.mode = mode

    def __enter__(self):
        self.prev = getattr(_forced, "mode", None)
        _forced.mode = self.mode

    def __exit__(self, *exc):
        _forced.mode = self.prev


def pack_conv_weight_bf16(w, transpose_flip=False):
    """(Cout,Cin,3,3) fp32 -> bf16 A-operand image of the bf16 MFMA kernel (round to nearest even)."""
    return _pack_single("odehip_pack_conv_weight_bf16", w, transpose_flip, torch.bfloat16, ks=3, per_pair=9,
                        ks_error="the bf16 kernel serves 3x3 layers only")


def pack_conv_weight_bf16_ks(w, transpose_flip=False):
    """(Cout,Cin,5,5) fp32 -> block-major bf16 image of the 5x5 bf16 ring kernel."""
    return _pack_single("odehip_pack_conv_weight_bf16_ks", w, transpose_flip, torch.bfloat16)


def pack_fused_bf16(convs, reverse_transposed=False):
    """Fused bf16 image of a stack of 64 -> 64 3x3 convs in execution order (the input-gradient chain runs the layers
    backwards with transposed + flipped weights)."""
    lib = _lib.load()
    n = len(convs)
    out = torch.empty(lib.odehip_fused_bf16_weight_bytes(n), dtype=torch.uint8, device=convs[0].weight.device)
    for e in range(n):
        c = convs[n - 1 - e] if reverse_transposed else convs[e]
        w = c.weight.detach().contiguous()
        require_device_tensor(w, "conv weight")
        _lib.check(lib.odehip_pack_convstack_fused_bf16(_ptr(w), _ptr(out), e, int(bool(reverse_transposed)), _stream()))
    return out


def _fusable(convs, ks):
    """bf16 mode, 64-channel 3x3 stacks: whole f in one launch (fstack_bf16.hip)."""
    return ks == 3 and all(c.in_channels == 64 and c.out_channels == 64 for c in convs)


def _bf16_cell_ok(cell_input, hidden, ks):
    return ks == 5 and cell_input % 16 == 0 and hidden % 32 == 0 and cell_input + hidden <= 128


def _bf16_ok(cin, cout, ks):
    return ks == 3 and cin % 16 == 0 and cin <= 128 and cin // 16 in (1, 2, 4, 8) and cout % 32 == 0


def conv_q4(src1, w_packed, bias, cout, ks, src2=None, relu=False, w_wino=None, w_bf16=None):
    """One conv layer on Q4 activations (tests / building block)."""
    require_device_tensor(src1, "src1")
    b = src1.shape[0]
    cin1 = src1.shape[1] * 4
    cin = cin1 + (src2.shape[1] * 4 if src2 is not None else 0)
    dst = torch.empty((b, cout // 4, 256, 4), dtype=torch.float32, device=src1.device)
    d = _lib.ConvDesc(src1=src1.data_ptr(), src2=src2.data_ptr() if src2 is not None else None, cin1=cin1, cin=cin,
                      cout=cout, ks=ks, batch=b, w_packed=w_packed.data_ptr(),
                      w_wino=w_wino.data_ptr() if w_wino is not None else None,
                      w_bf16=w_bf16.data_ptr() if w_bf16 is not None else None,
                      bias=bias.data_ptr() if bias is not None else None,
                      dst=dst.data_ptr(), relu=int(relu))
    _lib.check(_lib.load().odehip_conv_q4(ctypes.byref(d), _stream()))
    return dst


class PackedConvStack:
    """Packed weights of a `create_convnet` Sequential, refreshed when the live Parameters change
    (the optimizer updates them in place between calls: SURVEY.md section 8b, ownership)."""

    def __init__(self, convs, final_tanh=False, act=_lib.ACT_RELU):
        self.convs = list(convs)
        self.final_tanh = bool(final_tanh)
        self.act = int(act)   # hidden activation (_lib.ACT_RELU / ACT_TANH)
        self._cache = {}      # compute dtype -> dict(stamp, desc, keep, bias, dgrad = (desc, keep) of the input-gradient convs)
        self._bias = None
        self.desc = None

    def _current_stamp(self):
        return tuple((c.weight.data_ptr(), c.weight._version, c.bias.data_ptr(), c.bias._version) for c in self.convs)

    @property
    def relu_only(self):
        """ReLU between the convs and no Tanh head."""
        return self.act == _lib.ACT_RELU and not self.final_tanh

    @property
    def headless(self):
        """No Tanh head, ReLU or Tanh between the convs: the stacks the bf16 kernels implement."""
        return self.act in (_lib.ACT_RELU, _lib.ACT_TANH) and not self.final_tanh

    def refresh(self, mode=None):
        mode = mode or current_compute_dtype()
        if mode == "bf16" and not self.headless:   # checked per call: the compute dtype can change between calls on a cached stack
            raise TypeError("bf16 compute (set_compute_dtype('bf16') or autocast) supports dynamics without a Tanh head only "
                            "(final_act=False); this stack has a Tanh head: run it in fp32")
        if mode == "bf16" and self.act == _lib.ACT_TANH and not _bf16_tanh:   # (per call as well: the switch can change)
            raise TypeError("bf16 compute (set_compute_dtype('bf16') or autocast) runs Tanh dynamics only once they are switched on with "
                            "set_bf16_tanh(True): their derivative is then 1 - bf16(y)^2, not autograd's "
                            "1 - y^2.  Switch them on, or run this stack in fp32")
        stamp = self._current_stamp()
        ent = self._cache.get(mode)
        if ent is not None and ent["stamp"] == stamp:
            self.desc = ent["desc"]
            self._bias = ent["bias"]
            return ent["desc"]
        convs = self.convs
        if len(convs) > _lib.MAX_LAYERS:
            raise ValueError(f"at most {_lib.MAX_LAYERS} conv layers are supported")
        ks = convs[0].kernel_size[0]
        for c in convs:
            if c.kernel_size != (ks, ks) or c.stride != (1, 1) or c.padding != (ks // 2, ks // 2) or c.dilation != (1, 1) \
                    or c.groups != 1 or c.bias is None:
                raise ValueError("the HIP path supports stride-1 'same' square convs with bias only "
                                 f"(got {c}); downsize=True dynamics are not supported")
            require_device_tensor(c.weight, "conv weight")
        bias = [c.bias.detach().contiguous() for c in convs]
        d, keep = self._pack(mode, ks, bias, False)
        self._cache[mode] = dict(stamp=stamp, desc=d, keep=keep, bias=bias, dgrad=None)
        self.desc, self._bias = d, bias
        return d

    def _pack(self, mode, ks, bias, transpose_flip):
        """(ConvStack, the images it points to) of the convs in one direction: as they are, or transposed + flipped (the
        input-gradient convs: Cin and Cout swap roles, the fused image holds the layers in reverse order)."""
        convs = self.convs
        cin = [c.out_channels if transpose_flip else c.in_channels for c in convs]
        cout = [c.in_channels if transpose_flip else c.out_channels for c in convs]
        # 3x3 layers with cin % 16 == 0 run the Winograd kernel (2.25x fewer MFMAs, still exact-fp32 arithmetic)
        want_wino = [ks == 3 and ci % 16 == 0 for ci in cin]
        both = pack_conv_weights_many([(c.weight, False, transpose_flip) for c in convs] +
                                      [(c.weight, True, transpose_flip) for c, ww in zip(convs, want_wino) if ww])
        packed, rest = both[:len(convs)], iter(both[len(convs):])
        wino = [next(rest) if ww else None for ww in want_wino]
        bf16 = [pack_conv_weight_bf16(c.weight, transpose_flip) if mode == "bf16" and _bf16_ok(ci, co, ks) else None
                for c, ci, co in zip(convs, cin, cout)]
        fused = (pack_fused_bf16(convs, reverse_transposed=transpose_flip)
                 if mode == "bf16" and self.headless and _fusable(convs, ks) else None)
        d = _lib.ConvStack()
        d.w_fused = fused.data_ptr() if fused is not None else None
        d.n_convs = len(convs)
        d.ks = ks
        d.channels[0] = convs[0].in_channels
        for i, c in enumerate(convs):
            d.channels[i + 1] = c.out_channels
            d.w_packed[i] = packed[i].data_ptr()
            d.w_wino[i] = wino[i].data_ptr() if wino[i] is not None else None
            d.w_bf16[i] = bf16[i].data_ptr() if bf16[i] is not None else None
            d.bias[i] = bias[i].data_ptr()
        d.final_tanh = int(self.final_tanh)
        d.act = self.act
        return d, (packed, wino, bf16, fused)

    def dgrad_desc(self, mode=None):
        """Stack of the input-gradient convs (weights packed transposed + flipped), built on first use."""
        mode = mode or current_compute_dtype()
        d0 = self.refresh(mode)
        ent = self._cache[mode]
        if ent["dgrad"] is None:
            ent["dgrad"] = self._pack(mode, d0.ks, ent["bias"], True)
        return ent["dgrad"][0]


def convstack_forward(stack, y, negate=False):
    require_device_tensor(y, "y")
    desc = stack.refresh()
    y = y.contiguous()
    b = y.shape[0]
    if y.dim() != 4 or tuple(y.shape[2:]) != (16, 16) or y.shape[1] != desc.channels[0]:
        raise ValueError(f"y must be (B,{desc.channels[0]},16,16) (got {tuple(y.shape)})")
    lib = _lib.load()
    nbytes = lib.odehip_convstack_workspace_bytes(ctypes.byref(desc), b)
    ws = workspace(("f", b, tuple(desc.channels)), nbytes, y.device)
    out = torch.empty((b, desc.channels[desc.n_convs], 16, 16), dtype=torch.float32, device=y.device)
    _lib.check(lib.odehip_convstack_forward(ctypes.byref(desc), _ptr(y), _ptr(out), b, int(bool(negate)), _ptr(ws),
                                            ws.numel(), _stream()))
    return out


def _c_times(t):
    """The time grid as the c_double array the C ABI takes (len() of it = the number of time points)."""
    t64 = host_times(t).tolist()
    return (ctypes.c_double * len(t64))(*t64)


def _solver_inputs(stack, z0, t):
    """What every solver forward starts from: (refreshed descriptor, contiguous y0, batch, channels, time points, c_double time array)."""
    require_device_tensor(z0, "y0")
    desc = stack.refresh()
    z0 = z0.contiguous()
    b, c = z0.shape[0], z0.shape[1]
    if z0.dim() != 4 or tuple(z0.shape[2:]) != (16, 16) or c != desc.channels[0]:
        raise ValueError(f"y0 must be (B,{desc.channels[0]},16,16) (got {tuple(z0.shape)})")
    tarr = _c_times(t)
    return desc, z0, b, c, len(tarr), tarr


def _stack_grads(stack, batch, device):
    """Outputs of a solver backward: ((grad_z0, [grad_w...], [grad_b...]) -- what the wrappers return --, and the arrays of the weight
    and bias gradient pointers the C ABI takes)."""
    gz0 = torch.empty((batch, stack.desc.channels[0], 16, 16), dtype=torch.float32, device=device)
    gws = [torch.empty_like(cv.weight) for cv in stack.convs]
    gbs = [torch.empty_like(cv.bias) for cv in stack.convs]
    nl = len(gws)
    gw_arr = (ctypes.c_void_p * nl)(*[g.data_ptr() for g in gws])
    gb_arr = (ctypes.c_void_p * nl)(*[g.data_ptr() for g in gbs])
    return (gz0, gws, gbs), gw_arr, gb_arr


def odeint_fixed(stack, method, z0, t, save=False, negate=False):
    """Whole fixed-grid trajectory in one C-ABI call.  Returns (T,B,C,16,16); with save=True also the private
    workspace holding every saved activation (input of odeint_fixed_backward)."""
    desc, z0, b, c, n, tarr = _solver_inputs(stack, z0, t)
    lib = _lib.load()
    m = _lib.METHODS[method]
    nbytes = lib.odehip_odeint_workspace_bytes(ctypes.byref(desc), b, n, m, int(save))
    if save:  # private: it must survive untouched until backward
        ws = alloc_workspace(nbytes, z0.device)
    else:
        ws = workspace(("odeint", b, n, m, tuple(desc.channels)), nbytes, z0.device)
    out = torch.empty((n, b, c, 16, 16), dtype=torch.float32, device=z0.device)
    fmt = ctypes.c_int(0)
    if save and negate:   # a decreasing t under autograd (set_reverse_time_grads): the entry whose backward carries the sign
        _lib.check(lib.odehip_odeint_fixed_negated_saving(ctypes.byref(desc), m, _ptr(z0), tarr, n, b, _ptr(out), _ptr(ws), ws.numel(), _stream()))
        ws._odehip_saved_format = 0
        return out, ws
    _lib.check(lib.odehip_odeint_fixed(ctypes.byref(desc), m, _ptr(z0), tarr, n, b, _ptr(out), int(save), int(bool(negate)), _ptr(ws),
                                       ws.numel(), ctypes.byref(fmt), _stream()))
    if save:
        ws._odehip_saved_format = int(fmt.value)   # how the workspace holds the saved tensors (the backward call must be told)
    return (out, ws) if save else out


def odeint_fixed_backward(stack, method, t, batch, grad_out, ws, negate=False):
    """Gradients of the discrete fixed-grid solver: (grad_z0, [grad_w...], [grad_b...]).  negate: the forward was the negated solve
    (odeint_fixed(save=True, negate=True)); t is the increasing -t it ran on."""
    require_device_tensor(grad_out, "grad_out")
    desc = stack.refresh()
    dg = stack.dgrad_desc()
    grad_out = grad_out.contiguous()
    tarr = _c_times(t)
    grads, gw_arr, gb_arr = _stack_grads(stack, batch, grad_out.device)
    if negate:
        _lib.check(_lib.load().odehip_odeint_fixed_negated_backward(ctypes.byref(desc), ctypes.byref(dg), _lib.METHODS[method], tarr, len(tarr),
                                                                    batch, _ptr(grad_out), _ptr(grads[0]), gw_arr, gb_arr, _ptr(ws),
                                                                    ws.numel(), _stream()))
        return grads
    _lib.check(_lib.load().odehip_odeint_fixed_backward(ctypes.byref(desc), ctypes.byref(dg), _lib.METHODS[method], tarr, len(tarr),
                                                        batch, _ptr(grad_out), _ptr(grads[0]), gw_arr, gb_arr,
                                                        int(getattr(ws, "_odehip_saved_format", 0)), _ptr(ws), ws.numel(), _stream()))
    return grads


GRID_MAX_POINTS = 4096   # points of a time array the fixed-grid drivers take (csrc/fixed_grid.hip: check_common)
GRID_MAX_EVALS = 2048    # evaluations of f a saved trajectory may hold (the weight-gradient tables: csrc/fixed_grid.hip)
_STAGES = {"euler": 1, "midpoint": 2, "rk4": 4}


class EmitTable:
    """Which grid interval emits which output, as csrc/grid_interp.hip takes it (odehip_grid_emit_table).  Interval n = (grid[n],
    grid[n + 1]) emits the outputs first[n] <= j < first[n + 1]; exact[j]: t[j] is that interval's end point, the output is the grid
    state itself; slope[j]: fp32 weight of the interval's end state otherwise."""

    def __init__(self, n_grid, n_times):
        self.n_grid, self.n_times = n_grid, n_times
        self._first = (ctypes.c_int * n_grid)()
        self._slope = (ctypes.c_float * n_times)()
        self._exact = (ctypes.c_int * n_times)()

    first = property(lambda self: list(self._first))
    slope = property(lambda self: list(self._slope))
    exact = property(lambda self: [bool(e) for e in self._exact])


def grid_emit_table(grid, t):
    """The emit table of torchdiffeq's FixedGridODESolver.integrate for the internal `grid` and the requested (increasing) times `t`,
    built on the host by the library.  The grid must be one-dimensional, strictly increasing and run from t[0] to t[-1]:
    AssertionError otherwise, as torchdiffeq asserts."""
    gh, th = host_times(grid), host_times(t)
    if len(th) < 1 or len(gh) < 1:
        raise AssertionError("t and the grid must hold at least one point")
    if len(th) > 1 and not bool((th[1:] > th[:-1]).all()):
        raise AssertionError("t must be strictly increasing")
    if len(gh) > 1 and not bool((gh[1:] > gh[:-1]).all()):
        raise AssertionError("the grid of grid_constructor must be strictly increasing")
    if not (bool(gh[0] == th[0]) and bool(gh[-1] == th[-1])):
        raise AssertionError(f"the grid of grid_constructor must start at t[0] and end at t[-1] (grid {float(gh[0])} .. {float(gh[-1])}, "
                             f"t {float(th[0])} .. {float(th[-1])})")
    table = EmitTable(len(gh), len(th))
    _lib.check(_lib.load().odehip_grid_emit_table(_c_times(gh), len(gh), _c_times(th), len(th), table._first, table._slope, table._exact))
    return table


def _grid_call(fn, src, dst, table, state_floats):
    """One of the two launches of csrc/grid_interp.hip; the table travels into a workspace of its own."""
    lib = _lib.load()
    tab = workspace("grid_table", lib.odehip_grid_table_bytes(table.n_grid, table.n_times), src.device)
    _lib.check(getattr(lib, fn)(_ptr(src), _ptr(dst), table._first, table._slope, table._exact, table.n_grid, table.n_times, state_floats,
                                _ptr(tab), tab.numel(), _stream()))


def _same_times(grid, t):
    return grid.shape == t.shape and torch.equal(grid, t)


def odeint_fixed_on_grid(stack, method, z0, t, grid, save=False, negate=False):
    """odeint_fixed on an internal grid (torchdiffeq's grid_constructor): the solver steps through `grid`, the requested times `t`
    are filled by linear interpolation between the grid states around them -- one more launch (csrc/grid_interp.hip).  Returns what
    odeint_fixed returns, (T,B,C,16,16) and with save=True the workspace odeint_fixed_on_grid_backward takes.  A grid that equals t
    element for element is the plain call itself: no scratch, no extra launch.  The limits of the plain path hold for the G grid
    points: ValueError before any launch."""
    th, gh = host_times(t), host_times(grid)
    if _same_times(gh, th):
        return odeint_fixed(stack, method, z0, th, save=save, negate=negate)
    table = grid_emit_table(gh, th)
    g = len(gh)
    if g > GRID_MAX_POINTS:
        raise ValueError(f"odeint(HIP): a grid of G = {g} points exceeds the limit of {GRID_MAX_POINTS} points")
    if save and (g - 1) * _STAGES[method] > GRID_MAX_EVALS:
        raise ValueError(f"odeint(HIP): a grid of G = {g} points needs {(g - 1) * _STAGES[method]} evaluations of f under autograd; the "
                         f"backward pass keeps at most {GRID_MAX_EVALS} ((G - 1) * {_STAGES[method]} stages of {method})")
    res = odeint_fixed(stack, method, z0, gh, save=save, negate=negate)
    states = res[0] if save else res
    out = torch.empty((len(th),) + tuple(states.shape[1:]), dtype=torch.float32, device=states.device)
    _grid_call("odehip_grid_emit", states, out, table, states[0].numel())
    if save:
        res[1]._odehip_emit_table = table
        return out, res[1]
    return out


def odeint_fixed_on_grid_backward(stack, method, t, grid, batch, grad_out, ws, negate=False):
    """Gradients of odeint_fixed_on_grid: grad_out over the T outputs becomes a gradient over the G grid points (one launch, a gather
    per grid point: fixed order, no atomics), then the backward of the plain path runs on the grid with the saved workspace."""
    th, gh = host_times(t), host_times(grid)
    if _same_times(gh, th):
        return odeint_fixed_backward(stack, method, th, batch, grad_out, ws, negate=negate)
    require_device_tensor(grad_out, "grad_out")
    table = getattr(ws, "_odehip_emit_table", None) or grid_emit_table(gh, th)
    grad_out = grad_out.contiguous()
    if grad_out.shape[0] != len(th):
        raise ValueError(f"grad_out must hold {len(th)} frames (got {tuple(grad_out.shape)})")
    grad_grid = torch.empty((len(gh),) + tuple(grad_out.shape[1:]), dtype=torch.float32, device=grad_out.device)
    _grid_call("odehip_grid_scatter", grad_out, grad_grid, table, grad_out[0].numel())
    return odeint_fixed_backward(stack, method, gh, batch, grad_grid, ws, negate=negate)   # (the interpolation has no sign in it)


LOG_CAP = 2048   # accepted steps the forward reports back (the backward pass re-integrates them)


def _adaptive_code(method):
    """The C ABI's code of an adaptive method name ("dopri5", "bosh3").  bosh3 has no bf16 form: refused, not run in another mode."""
    if method not in _lib.ADAPTIVE_METHODS:
        raise ValueError(f"not an adaptive method of this path: {method!r}")
    if method == "bosh3" and current_compute_dtype() == "bf16":
        raise TypeError("odeint(HIP): method bosh3 is not implemented in bf16 compute mode (fp32 only); use dopri5 or "
                        'set_compute_dtype("f32")')
    return _lib.ADAPTIVE_METHODS[method]


def _dopri5_buffers(desc, z0, b, c, n, slots, m=_lib.DOPRI5):
    """(workspace, output) of an adaptive forward of method code m.  With `slots` the workspace also keeps the activations of that many
    accepted steps and is private (it must survive untouched until backward); without, it is the shared ("dopri5", ...) one."""
    lib = _lib.load()
    if slots:
        ws = alloc_workspace(lib.odehip_adaptive_saving_workspace_bytes(ctypes.byref(desc), b, n, slots, m), z0.device)
    else:
        ws = workspace(("dopri5", b, n, tuple(desc.channels)), lib.odehip_adaptive_workspace_bytes(ctypes.byref(desc), b, n, m), z0.device)
    return ws, torch.empty((n, b, c, 16, 16), dtype=torch.float32, device=z0.device)


def _dopri5_stats(stats, log, saved=None):
    """The stats dict of a dopri5 forward from what the library reported; `saved` (a c_int) adds whether activations were kept."""
    k = min(int(stats[1]), LOG_CAP)
    st = {"nfe": stats[0], "n_accept": stats[1], "n_reject": stats[2], "attempts_enqueued": stats[3],
          "accepted": [(log[2 * i], log[2 * i + 1]) for i in range(k)]}
    if saved is not None:
        st["saved"] = bool(saved.value)
    return st


def _c_step_log(accepted):
    """The accepted steps [(t0, dt), ...] as the flat c_double array the backward entry points take."""
    flat = [v for pair in accepted for v in pair]
    return (ctypes.c_double * max(len(flat), 1))(*flat)


def odeint_dopri5(stack, z0, t, rtol, atol, first_step=0.0, max_steps=0, negate=False, method="dopri5"):
    """Adaptive trajectory (method: "dopri5" or "bosh3"); returns ((T,B,C,16,16), stats dict).  stats["accepted"] = [(t0, dt), ...]."""
    m = _adaptive_code(method)
    collect_pending_solves()   # an asynchronous solve still in flight owns the shared ("dopri5", ...) workspace
    desc, z0, b, c, n, tarr = _solver_inputs(stack, z0, t)
    ws, out = _dopri5_buffers(desc, z0, b, c, n, 0, m)
    stats = (ctypes.c_int * 4)()
    log = (ctypes.c_double * (2 * LOG_CAP))()
    _lib.check(_lib.load().odehip_odeint_adaptive(m, ctypes.byref(desc), _ptr(z0), tarr, n, b, float(rtol), float(atol), float(first_step or 0.0),
                                                  int(max_steps), int(bool(negate)), _ptr(out), stats, log, LOG_CAP, _ptr(ws), ws.numel(),
                                                  _stream()))
    return out, _dopri5_stats(stats, log)


_dopri5_save_slots = 8   # slots of a saving forward's workspace; doubled (up to 64) after a forward that accepted more steps


def _grow_save_slots(slots, n_accept):
    """After a saving forward with `slots` slots that accepted n_accept steps: the next one gets room for them."""
    global _dopri5_save_slots
    if n_accept > slots:
        _dopri5_save_slots = min(64, max(2 * slots, n_accept + 2))


# ---- asynchronous dopri5 (include/odecgru_hip.h: odehip_odeint_dopri5_start / _collect) ------------------------------------------
# The synchronous entry points return when the device-side controller has reported completion, so the host cannot enqueue what comes
# BEHIND the solver meanwhile: in a whole training step (encoder -> solver -> decoder -> loss -> backward, ~600 launches) the device
# then idles while the backward pass is being enqueued (ODEConvGRU, B=64, dopri5: 20.9 ms per step against 12.1 ms of device work).
# With set_async_dopri5(True) a solve only ENQUEUES a few attempted steps and returns; its outcome (step counts, accepted-step log,
# whether activations were kept -- and any error: dt underflow, max_num_steps, non-finite state) is read when it is needed: at the
# backward pass, at the first look into ode_rl_amd.last_stats, or at the next dopri5 call.  Off by default: torchdiffeq raises such
# errors from odeint() itself, and so does the synchronous path.
_async_dopri5 = os.environ.get("ODEHIP_DOPRI5_ASYNC") == "1"
_async_attempts = 8      # attempted steps enqueued up front; follows what the previous solve needed (+ margin)
ASYNC_ATTEMPTS_MAX = 256
_pending_solves = []     # PendingDopri5 objects not collected yet


def set_async_dopri5(on=True):
    """Switch the asynchronous adaptive forward (dopri5 and bosh3) on / off (see above); returns the previous setting."""
    global _async_dopri5
    was = _async_dopri5
    _async_dopri5 = bool(on)
    if not on:
        collect_pending_solves()   # may raise a pending solve's error; the switch is already off then
    return was


def collect_pending_solves():
    """Wait for every dopri5 solve started asynchronously and surface its error, if any."""
    while _pending_solves:
        _pending_solves[0].collect()


class PendingDopri5:
    """A dopri5 solve that has been enqueued but whose outcome has not been read yet."""

    def __init__(self, token, keep, slots, ws):
        self.token, self._keep, self.slots, self.ws = token, keep, slots, ws
        self._result = None
        _pending_solves.append(self)

    def collect(self):
        """(stats dict, saved) -- saved = (workspace, slots) if the activations of the accepted steps were kept, else None."""
        global _async_attempts
        if isinstance(self._result, BaseException):   # the solve failed: every later look at it raises the same error
            raise self._result
        if self._result is None:
            if self in _pending_solves:
                _pending_solves.remove(self)
            stats = (ctypes.c_int * 4)()
            log = (ctypes.c_double * (2 * LOG_CAP))()
            saved = ctypes.c_int(0)
            lib = _lib.load()
            try:
                _lib.check(lib.odehip_odeint_dopri5_collect(int(self.token), stats, log, LOG_CAP, ctypes.byref(saved)))
            except _lib.AsyncSolveTruncated as e:
                # the attempts enqueued up front did not finish the solve and its consumers have read NaN frames: the NEXT solve gets
                # twice as many (the caller repeats its step; train_batch does)
                _async_attempts = min(ASYNC_ATTEMPTS_MAX, max(2 * int(stats[3]), _async_attempts))
                self._result = e
                raise
            except BaseException as e:
                self._result = e
                raise
            finally:
                self._keep = None
            if self.slots:
                _grow_save_slots(self.slots, int(stats[1]))
            # what this solve needed plus a margin of a quarter (at least 2): an attempt queued behind `done` costs three empty
            # launches, an attempt too few costs the step (AsyncSolveTruncated).  Never below what the last solve was given unless
            # it used less than half of it -- the count drifts slowly as the dynamics train
            used = int(stats[1]) + int(stats[2])
            want = used + max(2, used // 4)
            _async_attempts = max(4, min(ASYNC_ATTEMPTS_MAX, want if want > _async_attempts or 2 * want < _async_attempts else _async_attempts))
            self._result = (_dopri5_stats(stats, log, saved), (self.ws, self.slots) if saved.value else None)
            self.ws = None
        return self._result


class LazyStats(dict):
    """`ode_rl_amd.last_stats`: a dict that, after an asynchronous solve, fills itself on first access."""
    _pending = None

    def _bind(self, pending):
        dict.clear(self)
        self._pending = pending

    def _resolve(self):
        p, self._pending = self._pending, None
        if p is not None:
            dict.update(self, p.collect()[0])

    def clear(self):
        self._pending = None
        dict.clear(self)

    def __getitem__(self, k):
        self._resolve()
        return dict.__getitem__(self, k)

    def get(self, k, d=None):
        self._resolve()
        return dict.get(self, k, d)

    def __iter__(self):
        self._resolve()
        return dict.__iter__(self)

    def __len__(self):
        self._resolve()
        return dict.__len__(self)

    def __contains__(self, k):
        self._resolve()
        return dict.__contains__(self, k)

    def keys(self):
        self._resolve()
        return dict.keys(self)

    def items(self):
        self._resolve()
        return dict.items(self)

    def values(self):
        self._resolve()
        return dict.values(self)

    def copy(self):
        self._resolve()
        return dict(dict.items(self))

    def __eq__(self, other):
        self._resolve()
        return dict.__eq__(self, other)

    def __repr__(self):
        self._resolve()
        return dict.__repr__(self)


def odeint_dopri5_start(stack, z0, t, rtol, atol, first_step=0.0, max_steps=0, save=False, method="dopri5"):
    """Asynchronous dopri5 forward: returns (out, PendingDopri5) at once.  save=True keeps the activations of the accepted steps
    (as odeint_dopri5_saving does) in a private workspace held by the pending object."""
    m = _adaptive_code(method)
    collect_pending_solves()      # one solve in flight per process: the shared workspaces and the library's slots are free again
    desc, z0, b, c, n, tarr = _solver_inputs(stack, z0, t)
    slots = _dopri5_save_slots if save and os.environ.get("ODEHIP_DOPRI5_SAVE") != "0" else 0
    ws, out = _dopri5_buffers(desc, z0, b, c, n, slots, m)
    token = ctypes.c_int(-1)
    _lib.check(_lib.load().odehip_odeint_adaptive_start(m, ctypes.byref(desc), _ptr(z0), tarr, n, b, float(rtol), float(atol),
                                                      float(first_step or 0.0), int(max_steps), _ptr(out), int(slots), int(_async_attempts),
                                                      ctypes.byref(token), _ptr(ws), ws.numel(), _stream()))
    return out, PendingDopri5(token.value, (z0, out, ws), slots, ws if slots else None)


def odeint_dopri5_saving(stack, z0, t, rtol, atol, first_step=0.0, max_steps=0, method="dopri5", negate=False):
    """The forward of a dopri5 TRAINING step: odeint_dopri5 that also keeps the stage inputs and hidden activations of every accepted
    step in a private workspace, so that the backward pass needs no re-integration.  Returns (out, stats, saved) with saved =
    (workspace, max_accept), or None when nothing was kept (other stacks than 64-channel fp32, persistent walk off, more accepted
    steps than slots): the caller then takes odeint_dopri5_backward."""
    if _async_dopri5 and not negate:   # enqueue only: stats and `saved` are read later (LazyStats / PendingDopri5.collect())
        out, pending = odeint_dopri5_start(stack, z0, t, rtol, atol, first_step=first_step, max_steps=max_steps, save=True, method=method)
        return out, pending, pending
    if os.environ.get("ODEHIP_DOPRI5_SAVE") == "0":   # A/B switch: always re-integrate in the backward pass
        out, st = odeint_dopri5(stack, z0, t, rtol, atol, first_step=first_step, max_steps=max_steps, negate=negate, method=method)
        st["saved"] = False
        return out, st, None
    m = _adaptive_code(method)
    collect_pending_solves()
    desc, z0, b, c, n, tarr = _solver_inputs(stack, z0, t)
    slots = _dopri5_save_slots
    ws, out = _dopri5_buffers(desc, z0, b, c, n, slots, m)
    stats = (ctypes.c_int * 4)()
    log = (ctypes.c_double * (2 * LOG_CAP))()
    saved = ctypes.c_int(0)
    lib = _lib.load()
    entry = lib.odehip_odeint_adaptive_saving_negated if negate else lib.odehip_odeint_adaptive_saving
    _lib.check(entry(m, ctypes.byref(desc), _ptr(z0), tarr, n, b, float(rtol), float(atol),
                     float(first_step or 0.0), int(max_steps), _ptr(out), stats, log, LOG_CAP, slots, ctypes.byref(saved), _ptr(ws), ws.numel(),
                     _stream()))
    _grow_save_slots(slots, int(stats[1]))
    return out, _dopri5_stats(stats, log, saved), ((ws, slots) if saved.value else None)


def odeint_dopri5_backward_saved(stack, t, accepted, grad_out, saved, method="dopri5", negate=False):
    """Backward of odeint_dopri5_saving: the reverse sweep over the kept activations (no re-integration)."""
    require_device_tensor(grad_out, "grad_out")
    ws, slots = saved
    desc = stack.refresh()
    dg = stack.dgrad_desc()
    grad_out = grad_out.contiguous()
    tarr = _c_times(t)
    b = grad_out.shape[1]
    grads, gw_arr, gb_arr = _stack_grads(stack, b, grad_out.device)
    lib = _lib.load()
    entry = lib.odehip_odeint_adaptive_backward_saved_negated if negate else lib.odehip_odeint_adaptive_backward_saved
    _lib.check(entry(_adaptive_code(method), ctypes.byref(desc), ctypes.byref(dg), tarr, len(tarr), b, _c_step_log(accepted), len(accepted),
                     _ptr(grad_out), _ptr(grads[0]), gw_arr, gb_arr, int(slots), _ptr(ws), ws.numel(), _stream()))
    return grads


def odeint_dopri5_backward(stack, t, accepted, z0, grad_out, method="dopri5", negate=False):
    """Gradient of the accepted dopri5 steps (what autograd through torchdiffeq computes): (grad_z0, [grad_w], [grad_b])."""
    require_device_tensor(grad_out, "grad_out")
    require_device_tensor(z0, "y0")
    desc = stack.refresh()
    dg = stack.dgrad_desc()
    grad_out, z0 = grad_out.contiguous(), z0.contiguous()
    tarr = _c_times(t)
    n, b, ns = len(tarr), z0.shape[0], len(accepted)
    lib = _lib.load()
    m = _adaptive_code(method)
    nbytes = lib.odehip_adaptive_backward_workspace_bytes(ctypes.byref(desc), b, n, ns, m)
    # keyed WITHOUT the accepted-step count: that count drifts as the weights train, and a key per count would leave one
    # multi-GB buffer behind for every count ever seen; workspace() replaces a buffer that has become too small
    ws = workspace(("dopri5_bwd", b, n, tuple(desc.channels)), nbytes, grad_out.device)
    grads, gw_arr, gb_arr = _stack_grads(stack, b, grad_out.device)
    entry = lib.odehip_odeint_adaptive_backward_negated if negate else lib.odehip_odeint_adaptive_backward
    _lib.check(entry(m, ctypes.byref(desc), ctypes.byref(dg), tarr, n, b, _c_step_log(accepted), ns, _ptr(z0), _ptr(grad_out), _ptr(grads[0]),
                     gw_arr, gb_arr, _ptr(ws), ws.numel(), _stream()))
    return grads


def odeint_adjoint_backward(stack, method, t, y_traj, grad_out, negate=False):
    """torchdiffeq odeint_adjoint backward for the fixed-grid methods: (grad_z0, [grad_w...], [grad_b...]).  negate: y_traj is the
    trajectory of the negated solve on the increasing -t, which is `t` here."""
    require_device_tensor(grad_out, "grad_out")
    require_device_tensor(y_traj, "y_traj")
    desc = stack.refresh()
    dg = stack.dgrad_desc()
    grad_out, y_traj = grad_out.contiguous(), y_traj.contiguous()
    tarr = _c_times(t)
    n, b = len(tarr), y_traj.shape[1]
    lib = _lib.load()
    m = _lib.METHODS[method]
    nbytes = lib.odehip_odeint_workspace_bytes(ctypes.byref(desc), b, n, m, 1)
    ws = workspace(("adjoint", b, n, m, tuple(desc.channels)), nbytes, grad_out.device)
    grads, gw_arr, gb_arr = _stack_grads(stack, b, grad_out.device)
    entry = lib.odehip_odeint_adjoint_backward_negated if negate else lib.odehip_odeint_adjoint_backward
    _lib.check(entry(ctypes.byref(desc), ctypes.byref(dg), m, tarr, n, b, _ptr(y_traj), _ptr(grad_out), _ptr(grads[0]), gw_arr, gb_arr,
                     _ptr(ws), ws.numel(), _stream()))
    return grads


def adjoint_backward_grid(func, y_traj, method, t, options):
    """The grid of odeint_adjoint's backward pass under options["grid_constructor"], on the host: (grid, out_index).  torchdiffeq solves
    every backward interval (t[i], t[i-1]), i = T-1 .. 1, as an `odeint` call of its own with the caller's options: the decreasing pair
    is flipped to (-t[i], -t[i-1]) and the interval's grid is what odeint.internal_grid builds for that pair -- the constructor is called
    once per interval, in that order, with the state the interval starts from (y_traj[i], or None without a trajectory).  A grid of
    step_size_grid(h) is therefore anchored at t[i]: sub-steps of h back from t[i], the last one cut short at t[i-1].  `grid` joins the
    intervals' points in increasing time (float64, T <= G points), out_index[p] is the j with grid[p] == t[j] or -1 inside an interval.
    ValueError before any launch if the G points or their (G - 1) * stages evaluations of f exceed what the sweep holds."""
    from .odeint import internal_grid
    th = host_times(t)
    points, index = [th[-1:]], [len(th) - 1]   # walked backwards, in flipped time
    for i in range(len(th) - 1, 0, -1):
        pair = torch.stack([-th[i], -th[i - 1]])
        sub = internal_grid(func, None if y_traj is None else y_traj[i], pair, options)
        points.append(-sub[1:])
        index += [-1] * (len(sub) - 2) + [i - 1]
    grid = torch.cat(points).flip(0)
    g = len(grid)
    if g > GRID_MAX_POINTS:
        raise ValueError(f"odeint_adjoint(HIP): the backward grids hold G = {g} points, more than the limit of {GRID_MAX_POINTS} points")
    if (g - 1) * _STAGES[method] > GRID_MAX_EVALS:
        raise ValueError(f"odeint_adjoint(HIP): the backward grids hold G = {g} points, which needs {(g - 1) * _STAGES[method]} evaluations "
                         f"of f; the backward pass keeps at most {GRID_MAX_EVALS} ((G - 1) * {_STAGES[method]} stages of {method})")
    return grid, index[::-1]


def odeint_adjoint_on_grid_backward(stack, method, t, y_traj, grad_out, func, options):
    """odeint_adjoint_backward with torchdiffeq's `options` handed on to every backward interval (adjoint_backward_grid builds their
    grids): (grad_z0, [grad_w...], [grad_b...]).  Inside an interval the solver carries y itself; only at an output time is it reset
    to y_traj and does a_y take grad_out.  Intervals whose grids are their two end points make this odeint_adjoint_backward itself."""
    grid, index = adjoint_backward_grid(func, y_traj, method, t, options)
    th = host_times(t)
    if len(grid) == len(th):
        return odeint_adjoint_backward(stack, method, th, y_traj, grad_out)
    if current_compute_dtype() == "bf16":
        raise TypeError("odeint_adjoint(HIP): internal grids are not implemented in bf16 compute mode (fp32 only)")
    require_device_tensor(grad_out, "grad_out")
    require_device_tensor(y_traj, "y_traj")
    desc = stack.refresh()
    dg = stack.dgrad_desc()
    grad_out, y_traj = grad_out.contiguous(), y_traj.contiguous()
    tarr, garr = _c_times(th), _c_times(grid)
    n, g, b = len(tarr), len(garr), y_traj.shape[1]
    lib = _lib.load()
    m = _lib.METHODS[method]
    nbytes = lib.odehip_odeint_adjoint_grid_workspace_bytes(ctypes.byref(desc), b, n, g, m)
    ws = workspace(("adjoint_grid", b, n, m, tuple(desc.channels)), nbytes, grad_out.device)   # grows to the largest G met
    last_adjoint_grid.update(points=g, workspace_bytes=int(nbytes))
    grads, gw_arr, gb_arr = _stack_grads(stack, b, grad_out.device)
    _lib.check(lib.odehip_odeint_adjoint_backward_on_grid(ctypes.byref(desc), ctypes.byref(dg), m, tarr, n, garr, g,
                                                          (ctypes.c_int * g)(*index), b, _ptr(y_traj), _ptr(grad_out), _ptr(grads[0]),
                                                          gw_arr, gb_arr, _ptr(ws), ws.numel(), _stream()))
    return grads


_adjoint_grids = False   # odeint_adjoint takes odeint's internal grids (set_adjoint_grids)


def set_adjoint_grids(on=True):
    """Let odeint_adjoint take options={"grid_constructor": fn} for euler / midpoint / rk4 (off by default: the options are refused, as
    they always were).  On, the adjoint does what torchdiffeq's does -- a grid per BACKWARD interval, built from its flipped end points,
    so not the forward solve's grid (autograd.odeint_adjoint).  Returns the previous setting."""
    global _adjoint_grids
    was = _adjoint_grids
    _adjoint_grids = bool(on)
    return was


def adjoint_grids_enabled():
    return _adjoint_grids


_reverse_time_grads = False   # gradients through solves on a strictly decreasing t (set_reverse_time_grads)


def set_reverse_time_grads(on=True):
    """Let `odeint` under autograd and `odeint_adjoint` take a strictly decreasing t (off by default: both raise NotImplementedError, as
    they always did).  On, they differentiate what torchdiffeq differentiates there, the solve of dz/ds = -f(z) on s = -t: every
    method of `odeint`, with or without an internal grid, and the fixed-grid methods of `odeint_adjoint` without one; fp32 mode
    (TypeError in bf16 mode).  Returns the previous setting."""
    global _reverse_time_grads
    was = _reverse_time_grads
    _reverse_time_grads = bool(on)
    return was


def reverse_time_grads_enabled():
    return _reverse_time_grads


REVERSE_TIME_HINT = ("; gradients through a strictly decreasing t are opt-in: ode_rl_amd.set_reverse_time_grads(True) differentiates "
                     "the solve of the negated dynamics on -t, as torchdiffeq does")


last_adjoint_grid = {}   # points / workspace_bytes of the most recent gridded adjoint backward (instrumentation)


def odeint_adjoint_dopri5_backward(stack, t, y_traj, grad_out, rtol, atol, max_accept=None, stats=None, mixed_norm=False, method="dopri5"):
    """torchdiffeq odeint_adjoint backward with method="dopri5" or "bosh3" (seminorm, or the default mixed norm): (grad_z0, [grad_w...], [grad_b...]).
    `stats`, if a dict, receives nfe / n_accept / n_reject of the backward solve and `controller`: "device" when the device-steered
    seminorm path (csrc/adjoint_device.hip) took the call, "host" when the host-driven loop did."""
    m = _adaptive_code(method)
    collect_pending_solves()   # in particular the forward solve whose trajectory this integrates from (its error surfaces here)
    require_device_tensor(grad_out, "grad_out")
    require_device_tensor(y_traj, "y_traj")
    desc = stack.refresh()
    dg = stack.dgrad_desc()
    grad_out, y_traj = grad_out.contiguous(), y_traj.contiguous()
    tarr = _c_times(t)
    n, b = len(tarr), y_traj.shape[1]
    lib = _lib.load()
    if max_accept is None:  # every accepted step keeps its activations: default to what fits in 32 GiB, at most 256 steps
        per_step = (lib.odehip_adjoint_adaptive_workspace_bytes(ctypes.byref(desc), b, n, 2, m)
                    - lib.odehip_adjoint_adaptive_workspace_bytes(ctypes.byref(desc), b, n, 1, m))
        max_accept = int(max(4 * n, min(256, (32 << 30) // max(per_step, 1))))
    nbytes = lib.odehip_adjoint_adaptive_workspace_bytes(ctypes.byref(desc), b, n, int(max_accept), m)
    ws = workspace(("adjoint_dopri5", b, n, int(max_accept), tuple(desc.channels)), nbytes, grad_out.device)
    grads, gw_arr, gb_arr = _stack_grads(stack, b, grad_out.device)
    st = (ctypes.c_int * 3)()
    _lib.check(lib.odehip_odeint_adjoint_adaptive_backward(m, ctypes.byref(desc), ctypes.byref(dg), tarr, n, b, float(rtol),
                                                         float(atol), _ptr(y_traj), _ptr(grad_out), _ptr(grads[0]), gw_arr, gb_arr,
                                                         int(max_accept), int(bool(mixed_norm)), st, _ptr(ws), ws.numel(), _stream()))
    if stats is not None:
        stats.update(nfe=int(st[0]), n_accept=int(st[1]), n_reject=int(st[2]),
                     controller="device" if lib.odehip_last_adjoint_controller() == 1 else "host")
    return grads


class PackedCell:
    """Packed parameters of a ConvGRUCell (conv_gates / conv_can Sequentials), refreshed on parameter change; one cache entry
    per compute dtype (the bf16 entry adds the bf16 weight images of the two 5x5 convs)."""

    def __init__(self, cell):
        self.cell = cell
        self._cache = {}
        self._stamp = None     # identity of the entry returned last (keys the derived caches)
        self.desc = None

    @property
    def plain(self):
        """The norm-free cell of upstream Vid-ODE (models.conv_odegru.ConvGRUCell): conv_gates / conv_can are plain nn.Conv2d, reset gate
        first.  Its descriptor carries four NULL gn_* pointers and it has four parameters where the GroupNorm cell has eight."""
        return isinstance(self.cell.conv_gates, torch.nn.Conv2d)

    def _convs(self):
        c = self.cell
        return (c.conv_gates, c.conv_can) if self.plain else (c.conv_gates[0], c.conv_can[0])

    def _input_channels(self):
        return self._convs()[0].in_channels - self.cell.hidden_dim

    def _params(self):
        c = self.cell
        if self.plain:
            return [c.conv_gates.weight, c.conv_gates.bias, c.conv_can.weight, c.conv_can.bias]
        return [c.conv_gates[0].weight, c.conv_gates[0].bias, c.conv_gates[1].weight, c.conv_gates[1].bias,
                c.conv_can[0].weight, c.conv_can[0].bias, c.conv_can[1].weight, c.conv_can[1].bias]

    def grad_slots(self, grads):
        """The eight pointers of ConvGRUCellGrads / the cell part of EncoderGrads for `grads` (one tensor per _params() entry): a plain
        cell has no GroupNorm slots (NULL, never written)."""
        if self.plain:
            return [grads[0].data_ptr(), grads[1].data_ptr(), None, None, grads[2].data_ptr(), grads[3].data_ptr(), None, None]
        return [g.data_ptr() for g in grads]

    def refresh(self, mode=None):
        mode = mode or current_compute_dtype()
        plain = self.plain
        if plain and any(cv.bias is None for cv in self._convs()):
            raise ValueError("the HIP ConvGRU needs both convolutions to carry a bias (bias=True)")
        ps = self._params()
        stamp = (mode, winograd5_enabled()) + tuple((p.data_ptr(), p._version) for p in ps)
        ent = self._cache.get(mode)
        if ent is not None and ent[0] == stamp:
            self._stamp, self.desc = ent[0], ent[1]
            return ent[1]
        for p in ps:
            require_device_tensor(p, "ConvGRUCell parameter")
        c = self.cell
        conv_g, conv_c = self._convs()
        ks = conv_g.kernel_size[0]
        if any(tuple(cv.kernel_size) != (ks, ks) or tuple(cv.padding) != (ks // 2, ks // 2) or tuple(cv.stride) != (1, 1) for cv in (conv_g, conv_c)):
            raise ValueError("the HIP ConvGRU supports 'same' padding only")
        if plain:
            if c.hidden_dim % 32:
                raise ValueError(f"the HIP ConvGRU needs hidden_dim to be a multiple of 32 (got {c.hidden_dim})")
        elif c.conv_gates[1].num_groups * 32 != 2 * c.hidden_dim or c.conv_can[1].num_groups * 32 != c.hidden_dim:
            raise ValueError("the HIP ConvGRU needs GroupNorm groups of 32 channels (hidden_dim multiple of 32)")
        cin = self._input_channels()
        w_g, w_c = conv_g.weight, conv_c.weight
        want_wino = mode == "f32" and ks == 5 and winograd5_enabled() and cin % 8 == 0 and c.hidden_dim % 32 == 0
        packs = pack_conv_weights_many([(w_g, 0, False), (w_c, 0, False)] + ([(w_g, 2, False), (w_c, 2, False)] if want_wino else []))
        gn = [None] * 4 if plain else [ps[2].detach().contiguous(), ps[3].detach().contiguous(), ps[6].detach().contiguous(),
                                       ps[7].detach().contiguous()]
        keep = [packs[0], conv_g.bias.detach().contiguous(), gn[0], gn[1], packs[1], conv_c.bias.detach().contiguous(), gn[2], gn[3]]
        bf = [None, None]
        if mode == "bf16" and _bf16_cell_ok(cin, c.hidden_dim, ks):   # (5x5 only: a 3x3 cell runs fp32 in bf16 mode)
            bf = [pack_conv_weight_bf16_ks(w_g), pack_conv_weight_bf16_ks(w_c)]
        wino = packs[2:4] if want_wino else [None, None]
        keep = keep + wino
        ptr = [k.data_ptr() if k is not None else None for k in keep]
        d = _lib.ConvGRUCellDesc(input=cin, hidden=c.hidden_dim, ks=ks,
                                 w_gates_wino=ptr[8], w_can_wino=ptr[9],
                                 w_gates=ptr[0], b_gates=ptr[1], gn_gates_w=ptr[2], gn_gates_b=ptr[3], w_can=ptr[4], b_can=ptr[5],
                                 gn_can_w=ptr[6], gn_can_b=ptr[7],
                                 w_gates_bf16=bf[0].data_ptr() if bf[0] is not None else None,
                                 w_can_bf16=bf[1].data_ptr() if bf[1] is not None else None)
        self._cache[mode] = (stamp, d, keep, bf)
        self._stamp, self.desc = stamp, d
        return d

    def _half_slices(self):
        """The two conv weights cut into frame half and state half: gates-frame, gates-state, candidate-frame, candidate-state."""
        i = self._input_channels()
        wg, wc = (cv.weight.detach() for cv in self._convs())
        return [w.contiguous() for w in (wg[:, :i], wg[:, i:], wc[:, :i], wc[:, i:])]

    def bwd_desc(self):
        """The ConvGRUCellBwd of the entry refresh() returned last, packed once per stamp."""
        cached = getattr(self, "_bwd", None)
        if cached is None or cached[0] != self._stamp:
            keep, bf, wino = _cell_bwd_packs(self, self.desc, self._stamp[0])
            bw = _lib.ConvGRUCellBwd(*[k.data_ptr() for k in keep])
            _set_half_images(bw, bf, wino)
            cached = self._bwd = (self._stamp, bw, keep, bf, wino)
        return cached[1]


def _set_half_images(bw, bf, wino):
    """The optional bf16 / F(2x2,5x5) images of the four half slices into a backward descriptor (ConvGRUCellBwd, EncoderBwd)."""
    for j in range(4):
        bw.bf16[j] = bf[j].data_ptr() if bf[j] is not None else None
        bw.wino[j] = wino[j].data_ptr() if wino[j] is not None else None


def _cell_bwd_packs(packed_cell, d, mode, extra_jobs=()):
    """Transposed + flipped slices of the two 5x5 weights (frame half, state half), fp32 images and, in bf16 mode, bf16 ones; extra_jobs
    (pack_conv_weights_many tuples) ride in the same launch and their results follow the four slices in the first list."""
    slices = packed_cell._half_slices()
    want_wino = mode == "f32" and d.ks == 5 and winograd5_enabled() and all(w.shape[0] % 8 == 0 and w.shape[1] % 32 == 0 for w in slices)
    packs = pack_conv_weights_many([(w, 0, True) for w in slices] + list(extra_jobs) + ([(w, 2, True) for w in slices] if want_wino else []))
    keep, extra = packs[:4], packs[4:4 + len(extra_jobs)]
    bf = [None] * 4
    # only where the forward runs in bf16 too (_bf16_cell_ok): a cell the bf16 kernels do not serve stays fp32 in both directions
    if mode == "bf16" and d.ks == 5 and d.w_gates_bf16 and all(w.shape[0] <= 128 and w.shape[0] % 16 == 0 and w.shape[1] % 32 == 0 for w in slices):
        bf = [pack_conv_weight_bf16_ks(w, True) for w in slices]
    wino = packs[4 + len(extra_jobs):] if want_wino else [None] * 4
    return keep + extra, bf, wino


def convgru_cell_forward(packed_cell, x, h):
    require_device_tensor(x, "input_tensor")
    require_device_tensor(h, "h_cur")
    d = packed_cell.refresh()
    x, h = x.contiguous(), h.contiguous()
    b = x.shape[0]
    if tuple(x.shape) != (b, d.input, 16, 16) or tuple(h.shape) != (b, d.hidden, 16, 16):
        raise ValueError(f"ConvGRU step needs x (B,{d.input},16,16) and h (B,{d.hidden},16,16); got {tuple(x.shape)}, {tuple(h.shape)}")
    lib = _lib.load()
    nbytes = lib.odehip_convgru_cell_workspace_bytes(ctypes.byref(d), b)
    ws = workspace(("cgru", b, d.input, d.hidden), nbytes, x.device)
    out = torch.empty_like(h)
    _lib.check(lib.odehip_convgru_cell_forward(ctypes.byref(d), _ptr(x), _ptr(h), _ptr(out), b, _ptr(ws), ws.numel(), _stream()))
    return out


def convgru_cell_backward(packed_cell, x, h, grad_h_next):
    """Backward of one ConvGRU step: (grad_x, grad_h, [gradients of packed_cell._params()])."""
    for t_, n_ in ((x, "input_tensor"), (h, "h_cur"), (grad_h_next, "grad_h_next")):
        require_device_tensor(t_, n_)
    d = packed_cell.refresh()
    bw = packed_cell.bwd_desc()
    x, h, grad_h_next = x.contiguous(), h.contiguous(), grad_h_next.contiguous()
    b = x.shape[0]
    params = packed_cell._params()
    grads = [torch.empty_like(p) for p in params]
    g = _lib.ConvGRUCellGrads(*packed_cell.grad_slots(grads))
    gx, gh = torch.empty_like(x), torch.empty_like(h)
    lib = _lib.load()
    nbytes = lib.odehip_convgru_cell_backward_workspace_bytes(ctypes.byref(d), b)
    ws = workspace(("cgru_bwd", b, d.input, d.hidden), nbytes, x.device)
    _lib.check(lib.odehip_convgru_cell_backward(ctypes.byref(d), ctypes.byref(bw), _ptr(x), _ptr(h), _ptr(grad_h_next), _ptr(gx),
                                                _ptr(gh), ctypes.byref(g), b, _ptr(ws), ws.numel(), _stream()))
    return gx, gh, grads


def _cell_seq_desc(packed_cell):
    """(cell descriptor, odehip_convgru_cell_halves): the images of the two halves (frame, state) of the two 5x5 weights, each slice packed on its own: what
    the one-source steps of odehip_convgru_sequence_* run over.  Packed once per parameter version and compute dtype."""
    d = packed_cell.refresh()
    cached = getattr(packed_cell, "_seq", None)
    if cached is not None and cached[0] == packed_cell._stamp:
        return d, cached[1]
    mode = packed_cell._stamp[0]
    if d.ks != 5 or d.input % 8 or d.hidden % 32:
        raise ValueError(f"ConvGRU sequence: the 5x5 Winograd kernels serve kernel_size 5, input_dim % 8 == 0, hidden_dim % 32 == 0 "
                         f"(got {d.ks}, {d.input}, {d.hidden})")
    slices = packed_cell._half_slices()
    hv = _lib.ConvGRUCellHalves()
    if mode == "bf16":
        if not (_bf16_cell_ok(d.input, d.hidden, d.ks) and d.w_gates_bf16):
            raise ValueError(f"ConvGRU sequence: bf16 compute needs input_dim % 16 == 0, hidden_dim % 32 == 0 and input_dim + hidden_dim <= 128 "
                             f"(got {d.input}, {d.hidden})")
        keep = [pack_conv_weight_bf16_ks(w) for w in slices]
        for j in range(4):
            hv.bf16[j] = keep[j].data_ptr()
    else:
        if not d.w_gates_wino:
            raise ValueError("ConvGRU sequence: needs the F(2x2,5x5) form of the cell's weights (ODEHIP_WINO5=0 switches it off)")
        keep = pack_conv_weights_many([(w, 2, False) for w in slices])
        for j in range(4):
            hv.wino[j] = keep[j].data_ptr()
    packed_cell._seq = (packed_cell._stamp, hv, keep)
    return d, hv


def _check_sequence_args(d, x_seq, h0, n_steps):
    if x_seq is None and h0 is None:
        raise ValueError("ConvGRU sequence: input_tensor and h_cur are both None")
    n_steps = int(n_steps)
    if n_steps < 1:
        raise ValueError(f"ConvGRU sequence: seq_len must be at least 1 (got {n_steps})")
    b = None
    if x_seq is not None:
        require_device_tensor(x_seq, "input_tensor")
        if x_seq.dim() != 5 or x_seq.shape[0] < n_steps or tuple(x_seq.shape[2:]) != (d.input, 16, 16):
            raise ValueError(f"ConvGRU sequence: input_tensor must be (>= {n_steps},B,{d.input},16,16); got {tuple(x_seq.shape)}")
        b = x_seq.shape[1]
        x_seq = x_seq[:n_steps].detach().contiguous()
    if h0 is not None:
        require_device_tensor(h0, "h_cur")
        if h0.dim() != 4 or tuple(h0.shape[1:]) != (d.hidden, 16, 16) or (b is not None and h0.shape[0] != b):
            raise ValueError(f"ConvGRU sequence: h_cur must be (B,{d.hidden},16,16); got {tuple(h0.shape)}")
        b = h0.shape[0]
        h0 = h0.detach().contiguous()
    return x_seq, h0, n_steps, b


def convgru_sequence(packed_cell, x_seq, h0, n_steps, save=False):
    """n_steps ConvGRU steps in one call (csrc/convgru_sequence.hip).  x_seq (T,B,input,16,16) or None = zero input (one-source
    launches over the state half of the weights), h0 (B,hidden,16,16) or None = zero state.  Returns h_seq (T,B,hidden,16,16), written in
    place by the steps (the last state is h_seq[-1]); with save=True also what convgru_sequence_backward needs."""
    d, hv = _cell_seq_desc(packed_cell)
    x_seq, h0, n_steps, b = _check_sequence_args(d, x_seq, h0, n_steps)
    dev = (x_seq if x_seq is not None else h0).device
    lib = _lib.load()
    nbytes = lib.odehip_convgru_sequence_workspace_bytes(ctypes.byref(d), n_steps, b, int(x_seq is not None), int(bool(save)))
    if nbytes == 0:
        raise ValueError("ConvGRU sequence: bad sizes")
    # a training-mode forward owns its workspace until the backward pass has run
    ws = alloc_workspace(nbytes, dev) if save else workspace(("cgru_seq", n_steps, b, d.input, d.hidden, x_seq is not None), nbytes, dev)
    h_seq = torch.empty((n_steps, b, d.hidden, 16, 16), dtype=torch.float32, device=dev)
    fn = lib.odehip_convgru_sequence_train if save else lib.odehip_convgru_sequence_forward
    _lib.check(fn(ctypes.byref(d), ctypes.byref(hv), _ptr(x_seq), _ptr(h0), n_steps, b, _ptr(h_seq), _ptr(ws), ws.numel(), _stream()))
    if save:
        return h_seq, (ws, x_seq is not None, h0 is not None, n_steps, b, packed_cell._stamp)
    return h_seq


def convgru_sequence_backward(packed_cell, saved, grad_h_seq):
    """BPTT over a sequence convgru_sequence(save=True) ran: (grad_x_seq or None, grad_h0 or None, [gradients of packed_cell._params()]).
    Without x the frame half of the two conv weight gradients is exact zeros."""
    ws, has_x, has_h0, n_steps, b, stamp = saved
    require_device_tensor(grad_h_seq, "grad_h_seq")
    d, hv = _cell_seq_desc(packed_cell)
    if packed_cell._stamp != stamp:
        raise RuntimeError("a ConvGRUCell parameter (or the compute dtype) changed between the sequence's forward and its backward")
    bw = packed_cell.bwd_desc()
    grad_h_seq = grad_h_seq.contiguous()
    if tuple(grad_h_seq.shape) != (n_steps, b, d.hidden, 16, 16):
        raise ValueError(f"grad_h_seq must be ({n_steps},{b},{d.hidden},16,16); got {tuple(grad_h_seq.shape)}")
    dev = grad_h_seq.device
    grads = [torch.empty_like(p) for p in packed_cell._params()]
    g = _lib.ConvGRUCellGrads(*[t_.data_ptr() for t_ in grads])
    gx = torch.empty((n_steps, b, d.input, 16, 16), dtype=torch.float32, device=dev) if has_x else None
    gh0 = torch.empty((b, d.hidden, 16, 16), dtype=torch.float32, device=dev) if has_h0 else None
    _lib.check(_lib.load().odehip_convgru_sequence_backward(ctypes.byref(d), ctypes.byref(hv), ctypes.byref(bw), int(has_x), int(has_h0), n_steps, b,
                                                            _ptr(grad_h_seq), _ptr(gx), _ptr(gh0), ctypes.byref(g), _ptr(ws), ws.numel(),
                                                            _stream()))
    return gx, gh0, grads


class PackedEncoder:
    """Everything `ODEConvGRUCell.forward` needs on the device: encoder dynamics, cell, 1x1 head."""

    def __init__(self, f_stack, packed_cell, head):
        self.f_stack, self.packed_cell, self.head = f_stack, packed_cell, head
        self._stamp = None
        self._keep = None
        self.desc = None
        self.last_cell_steps = None            # steps for which the last forward call launched the cell (cell_steps_run)
        self.last_cell_steps_backward = None   # the same of the last backward call

    def refresh(self):
        fd = self.f_stack.refresh()
        cd = self.packed_cell.refresh()
        h0, h1 = self.head[0], self.head[2]
        ps = [h0.weight, h0.bias, h1.weight, h1.bias]
        stamp = (id(fd), id(cd)) + tuple((p.data_ptr(), p._version) for p in ps)
        if stamp == self._stamp:
            return self.desc
        hw = pack_conv_weights_many([(h0.weight, 0, False), (h1.weight, 0, False)])
        keep = [hw[0], h0.bias.detach().contiguous(), hw[1], h1.bias.detach().contiguous()]
        d = _lib.EncoderDesc()
        d.f_enc = fd
        d.cell = cd
        d.head_hidden = h0.out_channels
        d.out_ch = h1.out_channels // 2
        d.w_head0, d.b_head0, d.w_head1, d.b_head1 = (k.data_ptr() for k in keep)
        self._keep, self.desc, self._stamp = keep, d, stamp
        return d


def encoder_params(enc):
    """Parameters of the encoder in the order the training path returns their gradients."""
    ps = []
    for c in enc.f_stack.convs:
        ps += [c.weight, c.bias]
    return ps + enc.packed_cell._params() + [enc.head[0].weight, enc.head[0].bias, enc.head[2].weight, enc.head[2].bias]


def _encoder_bwd_desc(enc):
    """Transposed + flipped weight images of the input-gradient convs (rebuilt when a parameter changes)."""
    d = enc.refresh()
    stamp = enc._stamp
    cached = getattr(enc, "_bwd", None)
    if cached is not None and cached[0] is stamp:
        return cached[1]
    keep, bf, wino = _cell_bwd_packs(enc.packed_cell, d.cell, current_compute_dtype(),
                                     extra_jobs=[(enc.head[0].weight, 0, True), (enc.head[2].weight, 0, True)])
    b = _lib.EncoderBwd()
    b.f_dgrad = enc.f_stack.dgrad_desc()
    b.w_gates_dx, b.w_gates_dh, b.w_can_dx, b.w_can_dh, b.w_head0_t, b.w_head1_t = (k.data_ptr() for k in keep)
    _set_half_images(b, bf, wino)
    keep = keep + bf + wino
    enc._bwd = (stamp, b, keep)
    return b


def encoder_mask(mask, n_frames, batch, device, who="odeconvgru_encode"):
    """The observation mask as the library reads it: one contiguous float32 (T, B) tensor on `device`, or None.  mask: (B, T) or
    (B, T, 1), batch-first as the loaders make it, on the host or the device; mask[b, i] belongs to frame i of the time-first inputs.
    float32 values are used as they are (fractional masks blend), any other dtype is taken as mask != 0.  A constant: nothing is read
    back from it (no frame count, no host synchronisation), and a mask that requires grad is refused."""
    if mask is None:
        return None
    if not isinstance(mask, torch.Tensor):
        raise TypeError(f"{who}: mask must be a torch.Tensor or None (got {type(mask).__name__})")
    if mask.is_complex():
        raise TypeError(f"{who}: mask must be a real or boolean tensor (got {mask.dtype})")
    if mask.requires_grad:
        raise NotImplementedError(f"{who}: mask is treated as a constant; a gradient with respect to it is not implemented")
    if tuple(mask.shape) not in ((batch, n_frames), (batch, n_frames, 1)):
        raise ValueError(f"{who}: mask must be (B, T) = ({batch}, {n_frames}) (or with a trailing 1), batch-first; got {tuple(mask.shape)}")
    if mask.dtype != torch.float32:
        mask = mask != 0
    return mask.reshape(batch, n_frames).to(device=device, dtype=torch.float32).t().contiguous()


def _check_mask(mask, n_frames, batch, who):
    if not isinstance(mask, torch.Tensor):
        raise TypeError(f"{who}: mask must be a torch.Tensor or None (got {type(mask).__name__})")
    if mask.is_complex():
        raise TypeError(f"{who}: mask must be a real or boolean tensor (got {mask.dtype})")
    if tuple(mask.shape) not in ((batch, n_frames), (batch, n_frames, 1)):
        raise ValueError(f"{who}: mask must be (B, T) = ({batch}, {n_frames}) (or with a trailing 1), batch-first; got {tuple(mask.shape)}")


def observed_steps(mask, n_frames, batch, who="odeconvgru_encode"):
    """Which frames ANY sample observed, as the host step hint of the odehip_odeconvgru_encode*_steps calls: None or a length-T uint8
    numpy array, byte i = 1 iff mask[b, i] != 0 for some b (after encoder_mask's dtype rule: float32 as it is, so fractional values
    count and -0.0 does not; any other dtype as mask != 0).  Pure host code: a mask on the HOST is looked at where it is; a mask on the
    device gives None -- it is never read back -- and so does no mask.  mask: (B, T) or (B, T, 1) as for encoder_mask."""
    if mask is None:
        return None
    _check_mask(mask, n_frames, batch, who)
    if mask.device.type != "cpu":
        return None
    host = mask.detach()
    try:
        values = host.numpy()                # a view: a handful of numpy calls on B x T values, a few microseconds on the launch path
    except (TypeError, RuntimeError):        # a dtype numpy lacks (bfloat16)
        values = (host != 0).numpy()
    return np.ascontiguousarray((values.reshape(batch, n_frames) != 0).any(axis=0), dtype=np.uint8)


def encoder_steps(steps, mask, n_frames, batch, who="odeconvgru_encode"):
    """The `steps=` keyword of the encoder calls -> the host step hint (None or a length-T uint8 numpy array).  None (the default):
    derived from a host mask by observed_steps.  False: no hint, every step launches the cell.  A length-T sequence of booleans (list,
    numpy array, host tensor): the caller's own hint, with a device mask or with no mask at all -- a frame it switches off is computed
    as if its whole mask row were 0, whatever the mask says."""
    if steps is None or steps is True:
        return observed_steps(mask, n_frames, batch, who)
    if steps is False:
        return None
    if isinstance(steps, torch.Tensor):
        if steps.device.type != "cpu":
            raise TypeError(f"{who}: steps must live on the host (a list, a numpy array or a CPU tensor): a tensor on {steps.device} would "
                            "have to be read back, which costs the host synchronisation the hint exists to avoid")
        steps = steps.detach().numpy()
    arr = np.asarray(steps)
    if arr.ndim != 1 or arr.shape[0] != n_frames:
        raise ValueError(f"{who}: steps must be a sequence of T = {n_frames} booleans, one per frame; got shape {tuple(arr.shape)}")
    return np.ascontiguousarray(arr != 0, dtype=np.uint8)


def _steps_ptr(steps):
    return None if steps is None else steps.ctypes.data_as(ctypes.c_void_p)


def _encode(enc, inputs, timesteps, want_latent, run_backwards, train, mask=None, steps=None):
    """The encoder forward of both paths: (mean, std, latent_ys or None, what odeconvgru_encode_backward needs).  train: the entry point
    that keeps the per-frame activations, in a private workspace.  mask: see encoder_mask; None = every frame observed.  steps: see
    encoder_steps; the step count of the call goes to enc.last_cell_steps."""
    if isinstance(inputs, torch.Tensor) and inputs.dim() == 5:   # (mask and steps are refused before anything is built or launched)
        steps = encoder_steps(steps, mask, inputs.shape[0], inputs.shape[1])
        mask = encoder_mask(mask, inputs.shape[0], inputs.shape[1], inputs.device)
    require_device_tensor(inputs, "inputs")
    d = enc.refresh()
    inputs = inputs.contiguous()
    t, b, c = inputs.shape[0], inputs.shape[1], inputs.shape[2]
    if inputs.dim() != 5 or tuple(inputs.shape[3:]) != (16, 16) or c != d.cell.hidden:
        raise ValueError(f"inputs must be (T,B,{d.cell.hidden},16,16) time-first (got {tuple(inputs.shape)})")
    tarr = _c_times(timesteps)
    assert t == len(tarr), "Sequence length should be same as time_steps"
    lib = _lib.load()
    if train:
        ws = alloc_workspace(lib.odehip_encoder_train_workspace_bytes(ctypes.byref(d), t, b), inputs.device)   # owned by this call's graph node
        fn = lib.odehip_odeconvgru_encode_train_steps
    else:
        ws = workspace(("enc", t, b, c), lib.odehip_encoder_workspace_bytes(ctypes.byref(d), t, b), inputs.device)
        fn = lib.odehip_odeconvgru_encode_steps
    mean = torch.empty((b, d.out_ch, 16, 16), dtype=torch.float32, device=inputs.device)
    std = torch.empty_like(mean)
    latent = torch.empty((b, t, c, 16, 16), dtype=torch.float32, device=inputs.device) if want_latent else None
    n_run = ctypes.c_int(-1)
    _lib.check(fn(ctypes.byref(d), _ptr(inputs), tarr, t, b, int(bool(run_backwards)), _ptr(mean), _ptr(std), _ptr(latent), _ptr(ws),
                  ws.numel(), _stream(), _ptr(mask), _steps_ptr(steps), ctypes.byref(n_run)))
    enc.last_cell_steps = n_run.value
    return mean, std, latent, (ws, tarr, t, b, c, int(bool(run_backwards)), mask, steps)


def odeconvgru_encode_train(enc, inputs, timesteps, want_latent=False, run_backwards=True, mask=None, steps=None):
    """Forward of the training path: returns (mean, std, latent_ys or None, saved) -- `saved` holds the workspace the backward
    call needs, the (T, B) device image of `mask` and the host step hint (see encoder_steps), so the backward uses the forward's."""
    return _encode(enc, inputs, timesteps, want_latent, run_backwards, True, mask, steps)


def odeconvgru_encode_backward(enc, saved, grad_mean, grad_std, grad_latent=None, mask=None):
    """(grad_inputs (T,B,C,16,16), [gradient of every tensor of encoder_params(enc)]); grad_latent: what arrives through latent_ys.
    mask: the forward call's mask; None = the image of it that `saved` holds (none if the forward had none).  The step hint is the
    forward's (in `saved`); the number of steps whose cell kernels ran goes to enc.last_cell_steps_backward."""
    ws, tarr, t, b, c, run_backwards, mask_tb, steps = saved
    if mask is not None:
        mask_tb = encoder_mask(mask, t, b, ws.device, "odeconvgru_encode_backward")
    d = enc.refresh()
    bw = _encoder_bwd_desc(enc)
    dev = ws.device
    grad_mean = (torch.zeros((b, d.out_ch, 16, 16), device=dev) if grad_mean is None else grad_mean).contiguous()
    grad_std = (torch.zeros((b, d.out_ch, 16, 16), device=dev) if grad_std is None else grad_std).contiguous()
    require_device_tensor(grad_mean, "grad_mean")
    require_device_tensor(grad_std, "grad_std")
    if grad_latent is not None:
        grad_latent = grad_latent.contiguous()
        require_device_tensor(grad_latent, "grad_latent")
        if tuple(grad_latent.shape) != (b, t, c, 16, 16):
            raise ValueError(f"grad_latent must be ({b},{t},{c},16,16), got {tuple(grad_latent.shape)}")
    params = encoder_params(enc)
    grads = [torch.empty_like(p) for p in params]
    g = _lib.EncoderGrads()
    nl = len(enc.f_stack.convs)
    for l in range(nl):
        g.f_w[l] = grads[2 * l].data_ptr()
        g.f_b[l] = grads[2 * l + 1].data_ptr()
    (g.w_gates, g.b_gates, g.gn_gates_w, g.gn_gates_b, g.w_can, g.b_can, g.gn_can_w, g.gn_can_b) = enc.packed_cell.grad_slots(grads[2 * nl:-4])
    g.w_head0, g.b_head0, g.w_head1, g.b_head1 = (x.data_ptr() for x in grads[-4:])
    gin = torch.empty((t, b, c, 16, 16), dtype=torch.float32, device=dev)
    n_run = ctypes.c_int(-1)
    _lib.check(_lib.load().odehip_odeconvgru_encode_backward_steps(ctypes.byref(d), ctypes.byref(bw), tarr, t, b, run_backwards,
                                                                   _ptr(grad_mean), _ptr(grad_std), _ptr(grad_latent), _ptr(gin),
                                                                   ctypes.byref(g), _ptr(ws), ws.numel(), _stream(), _ptr(mask_tb),
                                                                   _steps_ptr(steps), ctypes.byref(n_run)))
    enc.last_cell_steps_backward = n_run.value
    return gin, grads


def odeconvgru_encode(enc, inputs, timesteps, want_latent=False, run_backwards=True, mask=None, steps=None):
    return _encode(enc, inputs, timesteps, want_latent, run_backwards, False, mask, steps)[:3]


# ---- VidODE's warp chain + mask compositing (csrc/warp.hip) ---------------------------------------------------------------
def warp_composite(pred_outputs, start_image, grid_x, grid_y):
    """pred_outputs (B,T,c+3,H,W), start_image (B,c,H,W) -> pred_x, warped (B,T,c,H,W), masks (B,T,1,H,W); one launch."""
    for t_, n_ in ((pred_outputs, "pred_outputs"), (start_image, "start_image"), (grid_x, "grid_x"), (grid_y, "grid_y")):
        require_device_tensor(t_, n_)
    pred_outputs, start_image = pred_outputs.contiguous(), start_image.contiguous()
    b, t, cc, h, w = pred_outputs.shape
    c = cc - 3
    if tuple(start_image.shape) != (b, c, h, w) or grid_x.numel() != w or grid_y.numel() != h:
        raise ValueError(f"warp_composite: start_image must be (B,{c},{h},{w}) and the grids ({w},), ({h},); got {tuple(start_image.shape)}")
    pred_x = torch.empty((b, t, c, h, w), dtype=torch.float32, device=pred_outputs.device)
    warped = torch.empty_like(pred_x)
    masks = torch.empty((b, t, 1, h, w), dtype=torch.float32, device=pred_outputs.device)
    _lib.check(_lib.load().odehip_warp_composite(_ptr(pred_outputs), _ptr(start_image), _ptr(grid_x.contiguous()), _ptr(grid_y.contiguous()),
                                                 b, t, c, h, w, _ptr(pred_x), _ptr(warped), _ptr(masks), _stream()))
    return pred_x, warped, masks


WARP_LDS_BYTES = 160 * 1024   # check_warp of csrc/warp.hip


def warp_backward_lds_bytes(channels, height, width):
    """LDS of csrc/warp.hip's backward: three (c, H, W) fp32 images -- the gradient that later steps produced, the one this step
    scatters, and the image the step sampled from (the forward holds two)."""
    return 3 * channels * height * width * 4


def warp_composite_backward_supported(channels, height, width):
    """Whether the backward runs where the forward does: at c = 4, 64 x 64 the forward's 128 KiB fit and the backward's 192 KiB do not."""
    return warp_backward_lds_bytes(channels, height, width) <= WARP_LDS_BYTES


def warp_composite_backward(pred_outputs, start_image, warped, grid_x, grid_y, g_pred_x, g_warped, g_masks, want_start_grad):
    b, t, cc, h, w = pred_outputs.shape
    c = cc - 3
    g_pred_x = (torch.zeros_like(warped) if g_pred_x is None else g_pred_x).contiguous()
    g_warped = g_warped.contiguous() if g_warped is not None else None
    g_masks = g_masks.contiguous() if g_masks is not None else None
    for t_ in (g_pred_x, g_warped, g_masks):
        if t_ is not None:
            require_device_tensor(t_, "gradient")
    g_po = torch.empty_like(pred_outputs)
    g_start = torch.empty_like(start_image) if want_start_grad else None
    _lib.check(_lib.load().odehip_warp_composite_backward(_ptr(pred_outputs), _ptr(start_image), _ptr(warped), _ptr(grid_x), _ptr(grid_y),
                                                          _ptr(g_pred_x), _ptr(g_warped), _ptr(g_masks), b, t, c, h, w, _ptr(g_po),
                                                          _ptr(g_start), _stream()))
    return g_po, g_start


def upsample2x(x):
    """nn.Upsample(scale_factor=2, mode='bilinear', align_corners=False) of an (..., H, W) fp32 device tensor (csrc/upsample.hip)."""
    require_device_tensor(x, "input")
    if x.dim() < 2 or x.shape[-1] % 2:
        raise ValueError(f"upsample2x: needs (..., H, W) with an even W, got {tuple(x.shape)}")
    x = x.contiguous()
    h, w = x.shape[-2:]
    out = torch.empty(tuple(x.shape[:-2]) + (2 * h, 2 * w), dtype=torch.float32, device=x.device)
    _lib.check(_lib.load().odehip_upsample2x_bilinear(_ptr(x), _ptr(out), x.numel() // (h * w), h, w, _stream()))
    return out


def upsample2x_backward(g):
    require_device_tensor(g, "gradient")
    g = g.contiguous()
    if g.dim() < 2 or g.shape[-2] % 2 or g.shape[-1] % 2:
        raise ValueError(f"upsample2x backward: needs (..., 2H, 2W), got {tuple(g.shape)}")
    h2, w2 = g.shape[-2:]
    gin = torch.empty(tuple(g.shape[:-2]) + (h2 // 2, w2 // 2), dtype=torch.float32, device=g.device)
    _lib.check(_lib.load().odehip_upsample2x_bilinear_backward(_ptr(g), _ptr(gin), gin.numel() // ((h2 // 2) * (w2 // 2)), h2 // 2, w2 // 2, _stream()))
    return gin


def bn_relu_up_forward(x, bn, upsample, conv_bias=None, group=None):
    """relu(bn(x)) [upsampled x2] in one pass (csrc/bn_relu_up.hip); bn: an nn.BatchNorm2d (its running statistics are updated in
    train() mode exactly as the module would).  Returns (out, saved) with saved = (mean, invstd, scale, shift) for the backward.
    group: a torch.distributed process group over which the batch is sharded (ode_rl_amd.dist.sync_batchnorm).  In train() mode the
    statistics are then those of the GLOBAL batch: the pass stops at its per-channel float64 sums [sum x | sum x^2 | count], ONE
    all-reduce on the current stream adds them over the ranks, and the pass resumes (shards may be uneven, not empty).  eval() mode
    needs no collective.  saved gains the reduced buffer's count for the backward.
    conv_bias: the bias of the convolution that produced x, NOT added to x (the caller ran the convolution without it).  A
    per-channel constant in front of BatchNorm cancels in train() mode -- only running_mean sees it -- and shifts the running mean in
    eval() mode: folding it here saves the bias-add pass over x and, in the backward, the reduction of a bias gradient that is exactly
    zero in train() mode (rocprofv3 of a VidODE step: 26 such convolutions, a 17-30 us add and a 40 us reduction each)."""
    require_device_tensor(x, "input")
    if x.dim() != 4 or x.shape[3] % 4:
        raise ValueError(f"bn_relu_up: needs (N, C, H, W) with W % 4 == 0, got {tuple(x.shape)}")
    if group is not None and x.shape[0] == 0:
        raise ValueError("bn_relu_up: this rank's shard of the batch is empty; cross-rank statistics need at least one sample per rank")
    x = x.contiguous()
    n, c, h, w = x.shape
    dev = x.device
    if bn.num_features != c or type(bn.momentum) is not float:   # (momentum=None -- a cumulative average -- is not built)
        raise ValueError(f"bn_relu_up: BatchNorm2d({bn.num_features}, momentum={bn.momentum}) on a {c}-channel input")
    for name in ("weight", "bias", "running_mean", "running_var"):
        p = getattr(bn, name)
        if p is not None:
            require_device_tensor(p, f"BatchNorm2d.{name}")
            if p.device != dev or p.numel() != c or not p.is_contiguous():
                raise ValueError(f"bn_relu_up: BatchNorm2d.{name} must be a contiguous ({c},) tensor on {dev}")
    if conv_bias is not None:
        require_device_tensor(conv_bias, "conv_bias")
        if conv_bias.device != dev or conv_bias.numel() != c or not conv_bias.is_contiguous():
            raise ValueError(f"bn_relu_up: conv_bias must be a contiguous ({c},) tensor on {dev}")
        conv_bias = conv_bias.detach()
    training = bn.training or bn.running_mean is None
    tracked = bn.track_running_stats and bn.running_mean is not None and bn.running_var is not None
    run_mean = bn.running_mean if tracked else None
    if conv_bias is not None and not training:
        run_mean = bn.running_mean - conv_bias      # (x + b - mean) = (x - (mean - b)); mean_out = this, so the backward's xhat agrees
    stats = torch.empty((4, c), dtype=torch.float32, device=dev)
    out = torch.empty((n, c, 2 * h, 2 * w) if upsample else (n, c, h, w), dtype=torch.float32, device=dev)
    lib = _lib.load()
    nws = lib.odehip_bn_workspace_bytes(c)
    ws = workspace(("bn", c), nws + 8 * c, dev)
    if training and bn.track_running_stats and bn.num_batches_tracked is not None:
        bn.num_batches_tracked.add_(1)
    saved = (stats, training)
    if group is not None and training:
        sums = torch.empty(2 * c + 1, dtype=torch.float64, device=dev)
        _lib.check(lib.odehip_bn_sync_stats(_ptr(x), n, c, h, w, _ptr(sums), _ptr(ws), ws.numel(), _stream()))
        torch.distributed.all_reduce(sums, op=torch.distributed.ReduceOp.SUM, group=group)
        _lib.check(lib.odehip_bn_sync_relu_up2x_forward(_ptr(x), n, c, h, w, _ptr(sums), _ptr(bn.weight), _ptr(bn.bias), _ptr(run_mean),
                                                        _ptr(bn.running_var) if tracked else None, float(bn.momentum), float(bn.eps),
                                                        int(bool(upsample)), _ptr(out), _ptr(stats[0]), _ptr(stats[1]), _ptr(stats[2]),
                                                        _ptr(stats[3]), _stream()))
        saved = (stats, training, sums[2 * c:])
    else:
        _lib.check(lib.odehip_bn_relu_up2x_forward(_ptr(x), n, c, h, w, _ptr(bn.weight), _ptr(bn.bias), _ptr(run_mean),
                                                   _ptr(bn.running_var) if tracked else None,
                                                   int(training), float(bn.momentum), float(bn.eps), int(bool(upsample)), _ptr(out),
                                                   _ptr(stats[0]), _ptr(stats[1]), _ptr(stats[2]), _ptr(stats[3]), _ptr(ws), ws.numel(),
                                                   _stream()))
    if conv_bias is not None and training and tracked:
        bn.running_mean.add_(conv_bias, alpha=bn.momentum)   # the mean of (x + b) is mean(x) + b
    return out, saved


def bn_relu_up_backward(grad_out, x, saved, upsample, group=None):
    """(grad_x, grad_weight, grad_bias).  group: the forward's.  In train() mode the two per-channel sums of the backward are then
    all-reduced (ONE collective) before dx; grad_weight / grad_bias stay this rank's sums, as nn.SyncBatchNorm returns them -- the
    gradient all-reduce of the step adds them up."""
    stats, training = saved[:2]
    require_device_tensor(grad_out, "gradient")
    grad_out, x = grad_out.contiguous(), x.contiguous()
    n, c, h, w = x.shape
    if tuple(grad_out.shape) != ((n, c, 2 * h, 2 * w) if upsample else (n, c, h, w)):
        raise ValueError(f"bn_relu_up backward: gradient of shape {tuple(grad_out.shape)} for an input of shape {tuple(x.shape)} (upsample={bool(upsample)})")
    dev = x.device
    lib = _lib.load()
    gx = torch.empty_like(x)
    g_pre = torch.empty_like(x)
    gw = torch.empty(c, dtype=torch.float32, device=dev)
    gb = torch.empty(c, dtype=torch.float32, device=dev)
    ws = workspace(("bn", c), lib.odehip_bn_workspace_bytes(c) + 8 * c, dev)
    if group is not None and training:
        if len(saved) != 3:
            raise ValueError("bn_relu_up backward: `group` given, but the forward ran without one")
        sums = torch.empty(2 * c, dtype=torch.float64, device=dev)
        _lib.check(lib.odehip_bn_sync_backward_sums(_ptr(grad_out), _ptr(x), n, c, h, w, _ptr(stats[0]), _ptr(stats[1]), _ptr(stats[2]),
                                                    _ptr(stats[3]), int(bool(upsample)), _ptr(g_pre), _ptr(gw), _ptr(gb), _ptr(sums), _ptr(ws),
                                                    ws.numel(), _stream()))
        torch.distributed.all_reduce(sums, op=torch.distributed.ReduceOp.SUM, group=group)
        _lib.check(lib.odehip_bn_sync_backward_apply(_ptr(g_pre), _ptr(x), n, c, h, w, _ptr(stats[0]), _ptr(stats[1]), _ptr(stats[2]), _ptr(sums),
                                                     _ptr(saved[2]), _ptr(gx), _ptr(ws), ws.numel(), _stream()))
        return gx, gw, gb
    if len(saved) == 3:
        raise ValueError("bn_relu_up backward: the forward reduced its statistics over a process group; pass the same `group`")
    _lib.check(lib.odehip_bn_relu_up2x_backward(_ptr(grad_out), _ptr(x), n, c, h, w, _ptr(stats[0]), _ptr(stats[1]), _ptr(stats[2]), _ptr(stats[3]),
                                                int(training), int(bool(upsample)), _ptr(gx), _ptr(gw), _ptr(gb), _ptr(g_pre), _ptr(ws), ws.numel(),
                                                _stream()))
    return gx, gw, gb


# ---- the conv encoder / decoder either side of the path (models/ODEConvGRU.py:101-140), one fused launch each ------------------
_codec_packs = {}   # id(module) -> (weakref to module, stamp, pack tensor)


def _codec_layers(seq, conv_type, kernel, n_mid):
    """The (conv, act, conv[, act]) structure of the reference's Encoder / Decoder with n_downs = n_ups = 2, or None."""
    mods = list(seq)
    if len(mods) not in (3, 4) or not isinstance(mods[0], conv_type) or not isinstance(mods[2], conv_type):
        return None
    if not all(isinstance(m, torch.nn.LeakyReLU) for m in mods[1::2]):
        return None
    c1, c2 = mods[0], mods[2]
    for c in (c1, c2):
        if c.kernel_size != (kernel, kernel) or c.stride != (2, 2) or c.padding != (1, 1) or c.bias is None or c.groups != 1 \
                or c.dilation != (1, 1) or (conv_type is torch.nn.ConvTranspose2d and c.output_padding != (0, 0)):
            return None
    if c1.out_channels != n_mid or c2.in_channels != n_mid or len({m.negative_slope for m in mods[1::2]}) != 1:
        return None
    return c1, c2, float(mods[1].negative_slope)


def frame_encoder_supported(seq):
    ls = _codec_layers(seq, torch.nn.Conv2d, 3, 16)
    return ls is not None and len(list(seq)) == 4 and 1 <= ls[0].in_channels <= 4 and ls[1].out_channels in (32, 64, 128)


def frame_decoder_supported(seq):
    ls = _codec_layers(seq, torch.nn.ConvTranspose2d, 4, 32)
    return ls is not None and len(list(seq)) == 3 and ls[0].in_channels in (32, 64, 128) and 1 <= ls[1].out_channels <= 4


def _codec_pack(seq, c1, c2, n_floats, pack_fn, in_ch, out_ch):
    params = (c1.weight, c1.bias, c2.weight, c2.bias)
    for p in params:
        require_device_tensor(p, "codec parameter")
    stamp = tuple((p.data_ptr(), p._version) for p in params)
    ent = _codec_packs.get(id(seq))
    if ent is not None and ent[0]() is seq and ent[1] == stamp:
        return ent[2]
    pack = torch.empty(int(n_floats), dtype=torch.float32, device=c1.weight.device)
    _lib.check(pack_fn(_ptr(c1.weight.detach().contiguous()), _ptr(c1.bias.detach().contiguous()), _ptr(c2.weight.detach().contiguous()),
                       _ptr(c2.bias.detach().contiguous()), in_ch, out_ch, _ptr(pack), _stream()))
    if len(_codec_packs) > 32:
        for k in [k for k, v in _codec_packs.items() if v[0]() is None]:
            del _codec_packs[k]
    _codec_packs[id(seq)] = (weakref.ref(seq), stamp, pack)
    return pack


def _frame_encoder_pack(seq, c1, c2):
    lib = _lib.load()
    return _codec_pack(seq, c1, c2, lib.odehip_frame_encoder_pack_floats(c1.in_channels, c2.out_channels), lib.odehip_pack_frame_encoder,
                       c1.in_channels, c2.out_channels)


def _frame_decoder_pack(seq, c1, c2):
    lib = _lib.load()
    return _codec_pack(seq, c1, c2, lib.odehip_frame_decoder_pack_floats(c1.in_channels, c2.out_channels), lib.odehip_pack_frame_decoder,
                       c1.in_channels, c2.out_channels)


def frame_encode(seq, frames):
    """`seq` = the reference Encoder's nn.Sequential (n_downs = 2).  frames (B,T,c,64,64) -> (T,B,out_ch,16,16) contiguous,
    TIME-FIRST: the layout ODEConvGRU.py:64-68 reaches through a permuted view."""
    require_device_tensor(frames, "frames")
    if not frame_encoder_supported(seq):
        raise ValueError("frame_encode: not the reference's Encoder structure (Conv2d 3/2/1 -> LeakyReLU -> Conv2d 3/2/1 -> LeakyReLU)")
    c1, c2, slope = _codec_layers(seq, torch.nn.Conv2d, 3, 16)
    if frames.dim() != 5 or frames.shape[2] != c1.in_channels or tuple(frames.shape[3:]) != (64, 64):
        raise ValueError(f"frame_encode: frames must be (B,T,{c1.in_channels},64,64), got {tuple(frames.shape)}")
    frames = frames.detach().contiguous()
    b, t = frames.shape[:2]
    pack = _frame_encoder_pack(seq, c1, c2)
    out = torch.empty((t, b, c2.out_channels, 16, 16), dtype=torch.float32, device=frames.device)
    _lib.check(_lib.load().odehip_frame_encode(_ptr(pack), _ptr(frames), b, t, c1.in_channels, c2.out_channels, slope, _ptr(out), _stream()))
    return out


def frame_decode(seq, latents, apply_sigmoid, save_mid=False):
    """`seq` = the reference Decoder's nn.Sequential (n_ups = 2).  latents (..., C, 16, 16) (any leading dims, e.g. the solver's
    (T,B)) -> (..., out_ch, 64, 64); apply_sigmoid folds the F.sigmoid of ODEConvGRU.py:85 into the launch.  save_mid: also return
    the 32-channel intermediate (N, 32 x 32 x 32 floats, the layout of odehip_frame_decode_train) for the backward pass."""
    require_device_tensor(latents, "latents")
    if not frame_decoder_supported(seq):
        raise ValueError("frame_decode: not the reference's Decoder structure (ConvTranspose2d 4/2/1 -> LeakyReLU -> ConvTranspose2d 4/2/1)")
    c1, c2, slope = _codec_layers(seq, torch.nn.ConvTranspose2d, 4, 32)
    if latents.dim() < 4 or latents.shape[-3] != c1.in_channels or tuple(latents.shape[-2:]) != (16, 16):
        raise ValueError(f"frame_decode: latents must be (...,{c1.in_channels},16,16), got {tuple(latents.shape)}")
    latents = latents.detach().contiguous()
    lead = tuple(latents.shape[:-3])
    n = 1
    for d in lead:
        n *= d
    pack = _frame_decoder_pack(seq, c1, c2)
    out = torch.empty(lead + (c2.out_channels, 64, 64), dtype=torch.float32, device=latents.device)
    mid = torch.empty((n, 32 * 32 * 32), dtype=torch.float32, device=latents.device) if save_mid else None
    _lib.check(_lib.load().odehip_frame_decode_train(_ptr(pack), _ptr(latents), n, c1.in_channels, c2.out_channels, slope,
                                                     1 if apply_sigmoid else 0, _ptr(out), _ptr(mid) if save_mid else None, _stream()))
    return (out, mid) if save_mid else out



def codec_backward_enabled():
    """ODEHIP_CODEC_BACKWARD=0: the frame encoder / decoder run as library calls under autograd (the behaviour before round 3)."""
    return os.environ.get("ODEHIP_CODEC_BACKWARD", "1") != "0"


def frame_encoder_backward_supported(seq):
    """The shapes csrc/frame_codec_backward.hip implements: one frame channel, 32 / 64 latent channels."""
    if not frame_encoder_supported(seq):
        return False
    c1, c2, _ = _codec_layers(seq, torch.nn.Conv2d, 3, 16)
    return c1.in_channels == 1 and c2.out_channels in (32, 64)


def frame_decoder_backward_supported(seq):
    if not frame_decoder_supported(seq):
        return False
    c1, c2, _ = _codec_layers(seq, torch.nn.ConvTranspose2d, 4, 32)
    return c2.out_channels == 1 and c1.in_channels in (32, 64)


def record_versions(ctx, params):
    """forward of an autograd Function whose backward reads the live parameters (it re-packs from them): remember which they were."""
    ctx.params = params
    ctx.versions = tuple(p._version for p in params)


def check_versions(ctx, subject):
    """backward: the parameters record_versions() saw must still be the forward's."""
    if tuple(p._version for p in ctx.params) != ctx.versions:
        raise RuntimeError(f"{subject} was modified in place between forward and backward")


def _codec_grads(c1, c2, ws_floats):
    """Outputs of a codec backward: the gradients of (c1.weight, c1.bias, c2.weight, c2.bias) and its float workspace."""
    grads = [torch.empty_like(p) for p in (c1.weight, c1.bias, c2.weight, c2.bias)]
    return grads, torch.empty(int(ws_floats), dtype=torch.float32, device=c1.weight.device)


class _FrameEncodeFn(torch.autograd.Function):
    """frame_encode under autograd: forward = the fused launch, backward = odehip_frame_encode_backward (gradients of the four
    parameter tensors; the frames carry none -- the caller checks that they do not ask for one)."""

    @staticmethod
    def forward(ctx, seq, frames, w1, b1, w2, b2):
        out = frame_encode(seq, frames)
        ctx.seq = seq
        record_versions(ctx, (w1, b1, w2, b2))
        ctx.save_for_backward(frames, out, w2)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        check_versions(ctx, "a parameter of the frame encoder")
        frames, out, w2 = ctx.saved_tensors
        c1, c2, slope = _codec_layers(ctx.seq, torch.nn.Conv2d, 3, 16)   # one frame channel (frame_encoder_backward_supported)
        lib = _lib.load()
        b, t = frames.shape[:2]
        pack = _frame_encoder_pack(ctx.seq, c1, c2)
        g = g.contiguous()
        frames = frames.detach().contiguous()
        (dw1, db1, dw2, db2), ws = _codec_grads(c1, c2, lib.odehip_frame_encode_backward_workspace_floats(b, t, 1, c2.out_channels))
        _lib.check(lib.odehip_frame_encode_backward(_ptr(pack), _ptr(w2.detach().contiguous()), _ptr(frames), _ptr(out), _ptr(g), b, t, 1,
                                                    c2.out_channels, slope, _ptr(dw1), _ptr(db1), _ptr(dw2), _ptr(db2), _ptr(ws), ws.numel(),
                                                    _stream()))
        return None, None, dw1, db1, dw2, db2


class _FrameDecodeFn(torch.autograd.Function):
    """frame_decode (+ sigmoid) under autograd: backward = odehip_frame_decode_backward (latents' and the four parameters' gradients)."""

    @staticmethod
    def forward(ctx, seq, latents, apply_sigmoid, w1, b1, w2, b2):
        # ODEHIP_CODEC_SAVE_MID=0: keep nothing but inputs and outputs, the backward recomputes the intermediate (32 KiB per image less
        # memory, ~0.1 ms more per 640 images)
        if os.environ.get("ODEHIP_CODEC_SAVE_MID", "1") != "0":
            pred, mid = frame_decode(seq, latents, apply_sigmoid, save_mid=True)
        else:
            pred, mid = frame_decode(seq, latents, apply_sigmoid), None
        ctx.seq, ctx.apply_sigmoid, ctx.has_mid = seq, bool(apply_sigmoid), mid is not None
        record_versions(ctx, (w1, b1, w2, b2))
        ctx.save_for_backward(latents, pred, w1, *([mid] if mid is not None else []))
        return pred

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        check_versions(ctx, "a parameter of the frame decoder")
        latents, pred, w1 = ctx.saved_tensors[:3]
        mid = ctx.saved_tensors[3] if ctx.has_mid else None
        c1, c2, slope = _codec_layers(ctx.seq, torch.nn.ConvTranspose2d, 4, 32)   # one frame channel (frame_decoder_backward_supported)
        lib = _lib.load()
        lat = latents.detach().contiguous()
        n = lat.numel() // (c1.in_channels * 256)
        pack = _frame_decoder_pack(ctx.seq, c1, c2)
        g = g.contiguous()
        g_lat = torch.empty_like(lat)
        (dw1, db1, dw2, db2), ws = _codec_grads(c1, c2, lib.odehip_frame_decode_backward_workspace_floats(n, c1.in_channels, 1))
        _lib.check(lib.odehip_frame_decode_backward(_ptr(pack), _ptr(w1.detach().contiguous()), _ptr(lat), _ptr(mid) if mid is not None else None,
                                                    _ptr(pred), _ptr(g), n, c1.in_channels, 1,
                                                    slope, 1 if ctx.apply_sigmoid else 0, _ptr(g_lat), _ptr(dw1), _ptr(db1), _ptr(dw2), _ptr(db2),
                                                    _ptr(ws), ws.numel(), _stream()))
        return None, g_lat.view_as(latents), None, dw1, db1, dw2, db2


def frame_encode_autograd(seq, frames):
    """frame_encode as a differentiable op of the encoder's parameters (frames must not require a gradient)."""
    if not frame_encoder_backward_supported(seq):
        raise ValueError("frame_encode_autograd: one frame channel and 32 / 64 latent channels only")
    if frames.requires_grad:
        raise ValueError("frame_encode_autograd: no gradient with respect to the frames (use the library path)")
    c1, c2, _ = _codec_layers(seq, torch.nn.Conv2d, 3, 16)
    return _FrameEncodeFn.apply(seq, frames, c1.weight, c1.bias, c2.weight, c2.bias)


def frame_decode_autograd(seq, latents, apply_sigmoid):
    """frame_decode as a differentiable op of the latents and the decoder's parameters."""
    if not frame_decoder_backward_supported(seq):
        raise ValueError("frame_decode_autograd: one frame channel and 32 / 64 latent channels only")
    c1, c2, _ = _codec_layers(seq, torch.nn.ConvTranspose2d, 4, 32)
    return _FrameDecodeFn.apply(seq, latents, apply_sigmoid, c1.weight, c1.bias, c2.weight, c2.bias)


def _check_latent_pair(mean, std, who):
    """mean, std: (B, C, 16, 16) float32 device tensors, C % 4 == 0 (what the solver takes as z0) -> (B, C)."""
    require_device_tensor(mean, "mean")
    require_device_tensor(std, "std")
    if mean.dim() != 4 or tuple(mean.shape[2:]) != (16, 16) or mean.shape[0] < 1 or mean.shape[1] < 4 or mean.shape[1] % 4:
        raise ValueError(f"{who}: mean must be (B, C, 16, 16) with C % 4 == 0, got {tuple(mean.shape)}")
    if std.shape != mean.shape or std.device != mean.device:
        raise ValueError(f"{who}: std must have mean's shape and device, got {tuple(std.shape)} on {std.device} for {tuple(mean.shape)} "
                         f"on {mean.device}")
    return mean.shape[0], mean.shape[1]


def _check_noise_rows(t, name, rows, ch, like, who):
    require_device_tensor(t, name)
    if tuple(t.shape) != (rows, ch, 16, 16) or t.device != like.device:
        raise ValueError(f"{who}: {name} must be ({rows}, {ch}, 16, 16) on {like.device}, got {tuple(t.shape)} on {t.device}")
    return t.detach().contiguous()


def latent_sample(mean, std, n_samples=1, seed=0, offset=0, batch_offset=0, global_batch=None, eps_in=None, want_kl=True, want_eps=False):
    """z0 = mean + std * eps for n_samples draws per batch row, and KL(N(mean, std) || N(0, 1)) per row, in ONE launch
    (csrc/latent_sample.hip).  Returns (z0 (K * B, C, 16, 16) sample-major, kl (B,) or None, eps (z0's shape) or None).  The noise is
    the counter-based stream of include/odecgru_hip.h (seed, offset; batch_offset / global_batch place this shard in the full batch)
    unless eps_in (z0's shape) brings the caller's own."""
    b, c = _check_latent_pair(mean, std, "latent_sample")
    k = int(n_samples)
    mean, std = mean.detach().contiguous(), std.detach().contiguous()
    if eps_in is not None:
        eps_in = _check_noise_rows(eps_in, "eps_in", k * b, c, mean, "latent_sample")
    z0 = torch.empty((k * b, c, 16, 16), dtype=torch.float32, device=mean.device)
    kl = torch.empty(b, dtype=torch.float32, device=mean.device) if want_kl else None
    eps = torch.empty_like(z0) if want_eps else None
    _lib.check(_lib.load().odehip_latent_sample(_ptr(mean), _ptr(std), b, c, 16, 16, k, int(seed), int(offset), int(batch_offset),
                                                b if global_batch is None else int(global_batch), _ptr(eps_in), _ptr(z0), _ptr(kl),
                                                _ptr(eps), _stream()))
    return z0, kl, eps


def latent_sample_backward(grad_z0, grad_kl, mean, std, n_samples=1, seed=0, offset=0, batch_offset=0, global_batch=None, eps_in=None):
    """(grad_mean, grad_std) of latent_sample from grad_z0 (K * B, C, 16, 16) and grad_kl ((B,) or None: no KL term), ONE launch; the
    noise is regenerated from the forward's (seed, offset, batch_offset, global_batch), or read from eps_in."""
    b, c = _check_latent_pair(mean, std, "latent_sample_backward")
    k = int(n_samples)
    mean, std = mean.detach().contiguous(), std.detach().contiguous()
    grad_z0 = _check_noise_rows(grad_z0, "grad_z0", k * b, c, mean, "latent_sample_backward")
    if eps_in is not None:
        eps_in = _check_noise_rows(eps_in, "eps_in", k * b, c, mean, "latent_sample_backward")
    if grad_kl is not None:
        require_device_tensor(grad_kl, "grad_kl")
        if tuple(grad_kl.shape) != (b,) or grad_kl.device != mean.device:
            raise ValueError(f"latent_sample_backward: grad_kl must be ({b},) on {mean.device}, got {tuple(grad_kl.shape)} on {grad_kl.device}")
        grad_kl = grad_kl.detach().contiguous()
    grad_mean, grad_std = torch.empty_like(mean), torch.empty_like(std)
    _lib.check(_lib.load().odehip_latent_sample_backward(_ptr(grad_z0), _ptr(grad_kl), _ptr(mean), _ptr(std), b, c, 16, 16, k, int(seed),
                                                         int(offset), int(batch_offset), b if global_batch is None else int(global_batch),
                                                         _ptr(eps_in), _ptr(grad_mean), _ptr(grad_std), _stream()))
    return grad_mean, grad_std


def fused_loss_enabled():
    """ODEHIP_FUSED_LOSS=0: the models' get_loss runs its torch composition on the GPU too (A/B against csrc/frame_loss.hip)."""
    return os.environ.get("ODEHIP_FUSED_LOSS", "1") != "0"


def _check_mse_pair(pred, truth, who):
    """pred (K * B, ...) and truth (B, ...) float32 device tensors with the same trailing shape, its size a multiple of 4
    -> (K, B, elements per row)."""
    require_device_tensor(pred, "pred")
    require_device_tensor(truth, "truth")
    if truth.dim() < 2 or truth.shape[0] < 1 or truth[0].numel() < 4 or truth[0].numel() % 4:
        raise ValueError(f"{who}: truth must be (B, ...) with a row size that is a positive multiple of 4, got {tuple(truth.shape)}")
    if pred.dim() != truth.dim() or pred.shape[1:] != truth.shape[1:] or pred.shape[0] < 1 or pred.shape[0] % truth.shape[0] or \
            pred.device != truth.device:
        raise ValueError(f"{who}: pred must be (K * B, ...) on truth's device with truth's trailing shape, got {tuple(pred.shape)} on "
                         f"{pred.device} for {tuple(truth.shape)} on {truth.device}")
    return pred.shape[0] // truth.shape[0], truth.shape[0], truth[0].numel()


def _check_device_scalar(t, name, like, who):
    require_device_tensor(t, name)
    if t.numel() != 1 or t.device != like.device:
        raise ValueError(f"{who}: {name} must hold one float on {like.device}, got {tuple(t.shape)} on {t.device}")
    return t.detach().contiguous()


def _check_kl(kl, b, like, who):
    require_device_tensor(kl, "kl")
    if tuple(kl.shape) != (b,) or kl.device != like.device:
        raise ValueError(f"{who}: kl must be ({b},) on {like.device}, got {tuple(kl.shape)} on {kl.device}")
    return kl.detach().contiguous()


def loss_mse(pred, truth, kl=None, kl_weight=1.0, kl_scale=0.0):
    """{loss, mse, kl_term} as a (3,) device tensor, two launches (csrc/frame_loss.hip): mse = mean (pred - truth)^2 with pred
    (K * B, ...) sample-major against truth (B, ...) -- row k * B + b against row b, the truth is not repeated --, kl_term =
    kl_scale * sum(kl) for kl (B,) or 0, loss = mse + kl_weight * kl_term.  Sums in float64, fixed order."""
    k, b, f = _check_mse_pair(pred, truth, "loss_mse")
    pred, truth = pred.detach().contiguous(), truth.detach().contiguous()
    if kl is not None:
        kl = _check_kl(kl, b, pred, "loss_mse")
    lib = _lib.load()
    ws = workspace("loss_mse", lib.odehip_loss_mse_workspace_bytes(k, b, f), pred.device)
    out = torch.empty(3, dtype=torch.float32, device=pred.device)
    _lib.check(lib.odehip_loss_mse(_ptr(pred), _ptr(truth), k, b, f, _ptr(kl), float(kl_scale), float(kl_weight), _ptr(out), _ptr(ws),
                                   ws.numel(), _stream()))
    return out


def loss_mse_backward(grad_out, pred, truth, kl_weight=1.0, kl_scale=0.0, want_kl=False):
    """(grad_pred, grad_kl or None) of loss_mse from grad_out, one float on the device, in ONE launch: grad_pred = (pred - truth) *
    (2 grad_out / N), grad_kl[b] = grad_out * kl_weight * kl_scale."""
    k, b, f = _check_mse_pair(pred, truth, "loss_mse_backward")
    pred, truth = pred.detach().contiguous(), truth.detach().contiguous()
    grad_out = _check_device_scalar(grad_out, "grad_out", pred, "loss_mse_backward")
    grad_pred = torch.empty_like(pred)
    grad_kl = torch.empty(b, dtype=torch.float32, device=pred.device) if want_kl else None
    _lib.check(_lib.load().odehip_loss_mse_backward(_ptr(grad_out), _ptr(pred), _ptr(truth), k, b, f, float(kl_scale), float(kl_weight),
                                                    _ptr(grad_pred), _ptr(grad_kl), _stream()))
    return grad_pred, grad_kl


def _frame_rows(t, name, lead, frame, who):
    """A float32 device tensor of shape lead + frame whose frames lie contiguous in memory, its leading strides multiples of 4 and
    its first element 16-byte aligned: as it is (a view is not copied), otherwise made contiguous."""
    require_device_tensor(t, name)
    if tuple(t.shape) != tuple(lead) + tuple(frame):
        raise ValueError(f"{who}: {name} must be {tuple(lead) + tuple(frame)}, got {tuple(t.shape)}")
    t = t.detach()
    n = len(lead)
    inner = t[(0,) * n]
    ok = inner.is_contiguous() and t.data_ptr() % 16 == 0 and all(s % 4 == 0 and s >= inner.numel() for s in t.stride()[:n])
    if ok and n == 2:   # frames of one batch row must not overlap the next row's
        ok = t.stride(0) >= t.stride(1) * (t.shape[1] - 1) + inner.numel()
    return t if ok else t.contiguous()


def _check_l1_args(pred, inter, truth, init, mask, who):
    """The tensors of the VidODE L1 pair, checked and laid out for the C ABI -> (pred, inter, truth, init, mask, mask_is_byte, B, T, n, P)."""
    require_device_tensor(pred, "pred")
    if pred.dim() < 3 or pred.shape[0] < 1 or pred.shape[1] < 1 or pred[0, 0].numel() < 4 or pred[0, 0].numel() % 4:
        raise ValueError(f"{who}: pred must be (B, n, ...) with a frame size that is a positive multiple of 4, got {tuple(pred.shape)}")
    b, n, frame = pred.shape[0], pred.shape[1], tuple(pred.shape[2:])
    require_device_tensor(truth, "truth")
    if truth.dim() != pred.dim() or truth.shape[0] != b or tuple(truth.shape[2:]) != frame or truth.shape[1] < n:
        raise ValueError(f"{who}: truth must be ({b}, T >= {n}) + {frame}, got {tuple(truth.shape)}")
    t = truth.shape[1]
    if not isinstance(mask, torch.Tensor):
        raise TypeError("mask must be a torch.Tensor")
    if mask.dim() == 3 and mask.shape[2] == 1:   # the loaders' (B, T, 1)
        mask = mask[:, :, 0]
    if tuple(mask.shape) != (b, t):
        raise ValueError(f"{who}: mask must be ({b}, {t}) or ({b}, {t}, 1), got {tuple(mask.shape)}")
    for name, x in (("inter", inter), ("init", init), ("mask", mask)):
        if isinstance(x, torch.Tensor) and x.device != pred.device:
            raise ValueError(f"{who}: {name} is on {x.device}, pred on {pred.device}")
    if not mask.is_cuda:
        raise RuntimeError(f"mask is on {mask.device}: the HIP path needs CUDA (ROCm) tensors and has no CPU fallback")
    mask = mask.detach()
    if mask.dtype not in (torch.float32, torch.uint8, torch.bool):
        mask = mask != 0
    mask = mask.contiguous()
    pred = _frame_rows(pred, "pred", (b, n), frame, who).contiguous()
    inter = _frame_rows(inter, "inter", (b, n), frame, who)
    truth = _frame_rows(truth, "truth", (b, t), frame, who).contiguous()
    init = _frame_rows(init, "init", (b,), frame, who)
    return pred, inter, truth, init, mask, 0 if mask.dtype == torch.float32 else 1, b, t, n, pred[0, 0].numel()


def _l1_call_args(pred, inter, truth, init, mask, mask_is_byte, b, t, n, p):
    """The arguments both VidODE L1 entry points take between grad_out and their outputs."""
    return (_ptr(pred), _ptr(inter), inter.stride(0), inter.stride(1), _ptr(truth), _ptr(init), init.stride(0), _ptr(mask), mask_is_byte,
            b, t, n, p)


def loss_vidode_l1(pred, inter, truth, init, mask):
    """{loss, l1_pred, l1_diff} of models/VidODE.py's get_loss as a (3,) device tensor, two launches, no host synchronisation
    (csrc/frame_loss.hip).  pred, inter (B, n, ...) -- inter may be a channel slice, it is not copied --, truth (B, T, ...), init
    (B, ...) the last observed frame (a view is fine), mask (B, T) or (B, T, 1), non-zero = selected, float32 / uint8 / bool as it is.
    l1_pred = mean |pred - truth[selected]|, l1_diff = mean |inter - (truth[t] - truth[t - 1])[selected]| with truth[-1] = init."""
    args = _check_l1_args(pred, inter, truth, init, mask, "loss_vidode_l1")
    b, n, p = args[6], args[8], args[9]
    lib = _lib.load()
    ws = workspace("loss_vidode_l1", lib.odehip_loss_vidode_l1_workspace_bytes(b, n, p), args[0].device)
    out = torch.empty(3, dtype=torch.float32, device=args[0].device)
    _lib.check(lib.odehip_loss_vidode_l1(*_l1_call_args(*args), _ptr(out), _ptr(ws), ws.numel(), _stream()))
    return out


def loss_vidode_l1_backward(grad_out, pred, inter, truth, init, mask):
    """(grad_pred, grad_inter), both (B, n, ...) contiguous, of loss_vidode_l1 from grad_out (one float on the device), ONE launch."""
    args = _check_l1_args(pred, inter, truth, init, mask, "loss_vidode_l1_backward")
    grad_out = _check_device_scalar(grad_out, "grad_out", args[0], "loss_vidode_l1_backward")
    grad_pred, grad_inter = torch.empty_like(args[0]), torch.empty_like(args[0])
    _lib.check(_lib.load().odehip_loss_vidode_l1_backward(_ptr(grad_out), *_l1_call_args(*args), _ptr(grad_pred), _ptr(grad_inter), _stream()))
    return grad_pred, grad_inter


def _check_planes(x, who):
    """x (N, C, ...) float32 on the device -> (contiguous x, planes = N * C, hw = elements per plane)."""
    require_device_tensor(x, "x")
    if x.dim() < 3 or x.shape[0] < 1 or x.shape[1] < 1:
        raise ValueError(f"{who}: x must be (N, C, ...) with at least one spatial dimension, got {tuple(x.shape)}")
    hw = x[0, 0].numel()
    if hw < 2:
        raise ValueError(f"{who}: expected more than 1 spatial element per plane, got input size {tuple(x.shape)}")
    return x.detach().contiguous(), x.shape[0] * x.shape[1], hw


def instnorm_lrelu(x, eps=1e-5, slope=0.2):
    """(y, mean, rstd) of InstanceNorm (no affine, biased variance) + LeakyReLU(slope) over the planes of x (N, C, ...): ONE launch
    (csrc/instnorm_act.hip).  mean, rstd (N * C,) are what instnorm_lrelu_backward needs besides x."""
    x, planes, hw = _check_planes(x, "instnorm_lrelu")
    y = torch.empty_like(x)
    mean = torch.empty(planes, dtype=torch.float32, device=x.device)
    rstd = torch.empty_like(mean)
    _lib.check(_lib.load().odehip_instnorm_lrelu_forward(_ptr(x), planes, hw, float(eps), float(slope), _ptr(y), _ptr(mean), _ptr(rstd), _stream()))
    return y, mean, rstd


def instnorm_lrelu_backward(grad_y, x, mean, rstd, slope=0.2):
    """grad_x of instnorm_lrelu from grad_y and the forward's x, mean, rstd: ONE launch."""
    x, planes, hw = _check_planes(x, "instnorm_lrelu_backward")
    require_device_tensor(grad_y, "grad_y")
    if grad_y.shape != x.shape or grad_y.device != x.device:
        raise ValueError(f"instnorm_lrelu_backward: grad_y must be {tuple(x.shape)} on {x.device}, got {tuple(grad_y.shape)} on {grad_y.device}")
    for name, s in (("mean", mean), ("rstd", rstd)):
        require_device_tensor(s, name)
        if tuple(s.shape) != (planes,) or s.device != x.device or not s.is_contiguous():
            raise ValueError(f"instnorm_lrelu_backward: {name} must be a contiguous ({planes},) on {x.device}, got {tuple(s.shape)} on {s.device}")
    grad_y = grad_y.detach().contiguous()
    grad_x = torch.empty_like(x)
    _lib.check(_lib.load().odehip_instnorm_lrelu_backward(_ptr(grad_y), _ptr(x), _ptr(mean), _ptr(rstd), planes, hw, float(slope), _ptr(grad_x),
                                                          _stream()))
    return grad_x


def gan_seq_len(t_in, t, interp=False):
    """L, the frames per row of gan_seq_assemble: t for the interpolation form (which needs t_in == t), else max(t, t_in + 1)."""
    if interp:
        if t_in != t:
            raise ValueError(f"gan_seq_assemble: the interpolation form needs as many observed frames as predictions, got {t_in} and {t}")
        return t
    return max(t, t_in + 1)


def _check_seq_pair(input_real, frames, who):
    require_device_tensor(input_real, "input_real")
    require_device_tensor(frames, "frames")
    if frames.dim() != 5 or input_real.dim() != 5 or input_real.shape[0] != frames.shape[0] or input_real.shape[2:] != frames.shape[2:] or \
            min(frames.shape) < 1 or input_real.shape[1] < 1 or input_real.device != frames.device:
        raise ValueError(f"{who}: input_real must be (b, t_in, c, h, w) and frames (b, t, c, h, w) on one device, got {tuple(input_real.shape)} on "
                         f"{input_real.device} and {tuple(frames.shape)} on {frames.device}")


def gan_seq_assemble(input_real, frames, interp=False):
    """The rows the sequence discriminator judges, (t * b, L * c, h, w), from input_real (b, t_in, c, h, w) and frames (b, t, c, h, w) in ONE
    launch (csrc/gan.hip).  Row i * b + n: [zeros] ++ input_real[n, i:] ++ frames[n, :i+1] right-aligned in L = max(t, t_in + 1) frames, or
    with interp=True input_real[n] with frame i replaced by frames[n, i]."""
    _check_seq_pair(input_real, frames, "gan_seq_assemble")
    b, t, c, h, w = frames.shape
    t_in = input_real.shape[1]
    seq = gan_seq_len(t_in, t, interp)
    input_real, frames = input_real.detach().contiguous(), frames.detach().contiguous()
    out = torch.empty((t * b, seq * c, h, w), dtype=torch.float32, device=frames.device)
    _lib.check(_lib.load().odehip_gan_seq_assemble(_ptr(input_real), _ptr(frames), b, t_in, t, c * h * w, int(bool(interp)), _ptr(out), _stream()))
    return out


def gan_seq_assemble_backward(grad_out, shape, t_in, interp=False):
    """grad_frames (b, t, c, h, w) = `shape` of gan_seq_assemble from grad_out (t * b, L * c, h, w): ONE launch, a gather."""
    b, t, c, h, w = shape
    seq = gan_seq_len(t_in, t, interp)
    require_device_tensor(grad_out, "grad_out")
    if tuple(grad_out.shape) != (t * b, seq * c, h, w):
        raise ValueError(f"gan_seq_assemble_backward: grad_out must be {(t * b, seq * c, h, w)}, got {tuple(grad_out.shape)}")
    grad_out = grad_out.detach().contiguous()
    grad_frames = torch.empty(tuple(shape), dtype=torch.float32, device=grad_out.device)
    _lib.check(_lib.load().odehip_gan_seq_assemble_backward(_ptr(grad_out), b, t_in, t, c * h * w, int(bool(interp)), _ptr(grad_frames), _stream()))
    return grad_frames


def loss_lsgan(pred, target):
    """mean (pred - target)^2 as a () device tensor, two launches, float64 sums in a fixed order (csrc/gan.hip)."""
    require_device_tensor(pred, "pred")
    if pred.numel() < 1:
        raise ValueError("loss_lsgan: pred is empty")
    pred = pred.detach().contiguous()
    lib = _lib.load()
    ws = workspace("loss_lsgan", lib.odehip_loss_lsgan_workspace_bytes(pred.numel()), pred.device)
    out = torch.empty((), dtype=torch.float32, device=pred.device)
    _lib.check(lib.odehip_loss_lsgan(_ptr(pred), pred.numel(), float(target), _ptr(out), _ptr(ws), _stream()))
    return out


def loss_lsgan_backward(grad_out, pred, target):
    """grad_pred = grad_out * 2 (pred - target) / n from grad_out, one float on the device, in ONE launch."""
    require_device_tensor(pred, "pred")
    if pred.numel() < 1:
        raise ValueError("loss_lsgan_backward: pred is empty")
    pred = pred.detach().contiguous()
    grad_out = _check_device_scalar(grad_out, "grad_out", pred, "loss_lsgan_backward")
    grad = torch.empty_like(pred)
    _lib.check(_lib.load().odehip_loss_lsgan_backward(_ptr(grad_out), _ptr(pred), pred.numel(), float(target), _ptr(grad), _stream()))
    return grad
