"""Cases of the forward-convolution shape tests (test_hip_conv_shapes.py): the tables, the procedural values and the CPU references.

A layer case is (b, cin1, cin2, cout, ks, relu, bias): a conv over cat(src1, src2) (cin2 = 0: one source) on 16x16 maps.  Values are
procedural: inputs in [-1, 1), weights uniform within +-1/sqrt(cin ks^2), a bias in [-1, 1) (None where `bias` is False).  The reference
is F.conv2d in float64 on the CPU (bf16 cases: operands rounded to bf16 first, the bias kept); `d32` is the rel-L2 distance of the same
conv in float32 from it, and every case must satisfy 4 * d32 <= the bound of its family (a condition on the reference alone)."""
import functools
import zlib

import torch
import torch.nn.functional as F

from conftest import procedural_tensor, rel_l2

# rel-L2 bounds per kernel family: those of test_hip_conv.py and test_hip_bf16.py
BOUND = {"direct": 2e-6, "wino3": 5e-6, "wino5": 1e-5, "bf16": 1e-5}

# ---- A: direct fp32 kernels (w_packed only)
DIRECT = [
    (2, 48, 0, 32, 3, True, True),      # conv3x3_resident_kernel<3>
    (1, 80, 0, 64, 3, False, True),     # 3x3 ring, 5 chunks = NBUF
    (2, 96, 0, 96, 3, True, True),      # 3x3 ring, 6 chunks (first wrap), cout 96
    (1, 256, 0, 32, 3, False, True),    # 3x3 ring, 16 chunks
    (3, 16, 32, 64, 3, False, True),    # two-source 3x3 ring, 3 chunks < NBUF, boundary on a chunk edge
    (2, 8, 40, 32, 3, True, True),      # two-source, boundary inside the first chunk
    (2, 72, 56, 32, 3, False, True),    # two-source, 8 chunks, boundary inside chunk 4
    (2, 64, 0, 64, 3, True, False),     # ReLU without a bias
    (2, 16, 0, 32, 1, False, True),     # 1x1, 1 chunk
    (2, 48, 0, 64, 1, True, True),      # 1x1, 3 chunks
    (1, 128, 0, 32, 1, False, True),    # 1x1, 8 chunks (wrap)
    (2, 8, 56, 64, 1, False, True),     # two-source 1x1, boundary inside a chunk
    (1, 192, 0, 96, 1, True, True),     # 1x1, 12 chunks, cout 96
    (2, 16, 0, 32, 5, False, True),     # 5x5 ring, 2 chunks
    (2, 24, 0, 32, 5, True, True),      # 5x5 ring, 3 chunks
    (1, 40, 0, 160, 5, False, True),    # 5x5 ring, 5 chunks, cout 160
    (2, 8, 32, 64, 5, False, True),     # 5x5, unequal sources
    (2, 12, 20, 32, 5, True, True),     # 5x5, q1 odd: boundary inside a chunk
    (17, 24, 0, 256, 5, False, True),   # conv_ring_kernel<5,1,2,2> (grid 272 > 256), odd chunk count on NBUF = 2
    (33, 8, 16, 128, 5, True, True),    # the same kernel (grid 264), two sources
]

# ---- B: Winograd F(2x2,3x3) (w_wino given)
WINO3_RUN = [
    (2, 48, 0, 64, 3, False, True),     # conv3x3_wino_kernel<3>
    (1, 48, 0, 96, 3, True, True),      # conv3x3_wino_kernel<3>, cout 96
    (1, 64, 0, 96, 3, False, True),     # conv3x3_wino_kernel<4>, odd tile-pair count
]
WINO3_DECLINE = [                       # rows of table A: no instantiation for 5 / 6 / 16 chunks, none for two sources
    (1, 80, 0, 64, 3, False, True),
    (2, 96, 0, 96, 3, True, True),
    (1, 256, 0, 32, 3, False, True),
    (3, 16, 32, 64, 3, False, True),
]
# input gradients of a (cin -> cout) layer: (b, cin, cout, family).  32 -> 96: the 96 -> 32 conv has no Winograd instantiation (ring
# kernel); 64 -> 32: the 32 -> 64 conv takes conv3x3_wino_kernel<2>
WINO3_DGRAD = [(2, 32, 96, "direct"), (2, 64, 32, "wino3")]

# ---- C: Winograd F(2x2,5x5) (w_wino from pack_conv_weight_winograd5): (b, cin1, cin2, cout) -> (split count S, chunks per share)
WINO5 = {
    (1, 24, 0, 32): (1, 3),             # unsplit, 3 chunks
    (1, 48, 0, 32): (2, 3),
    (1, 16, 16, 96): (2, 2),            # cout 96
    (1, 32, 64, 32): (4, 3),            # source boundary inside share 1
    (1, 40, 120, 32): (4, 5),
    (1, 64, 128, 64): (8, 3),
    (2, 8, 32, 32): (1, 5),             # unsplit, unequal sources
}
WINO5_DECLINE = (2, 12, 20, 32)         # q1 odd: the direct kernel
WINO5_DGRAD = (2, 32, 32, 96)           # input gradient of a (32+32) -> 96 layer: a 96 -> 64 conv, 12 chunks, S = 4


def wino5_split(b, cin, cout):
    """(S, chunks per share) as launch_wino5 chooses them: the largest S in (8, 4, 2) whose workgroups all fit the chip at once, that
    divides the cin / 8 chunks and leaves every share at least two of them; else one workgroup per tile."""
    nchunk = cin // 8
    s = next((k for k in (8, 4, 2) if (cout // 32) * 2 * b * k <= 256 and nchunk % k == 0 and nchunk // k >= 2), 1)
    return s, nchunk // s


# ---- D: bf16 single layers (w_bf16 given)
BF16_3X3_RUN = [(2, 16, 0, 32, 3, False, True), (3, 32, 0, 96, 3, True, True)]            # conv3x3_bf16_kernel<1>, <2>
BF16_3X3_DECLINE = [(2, 48, 0, 32, 3, True, True), (2, 96, 0, 96, 3, True, True), (3, 16, 32, 64, 3, False, True)]   # rows of table A
BF16_5X5_RUN = [(2, 16, 0, 32, 5, False, True), (1, 16, 32, 64, 5, False, True), (2, 48, 64, 32, 5, False, True),
                (1, 64, 64, 96, 5, False, True), (1, 160, 0, 32, 5, False, True)]         # the last: the last cin under the LDS bound
BF16_5X5_OVER_LDS = (1, 176, 0, 32, 5, False, True)     # the first cin over it: packs, the launch declines
BF16_5X5_PACK_REFUSES = (2, 24, 0, 32, 5, True, True)   # cin % 16 != 0: a row of table A; the pack refuses it

# ---- E: ConvGRU cells (input, hidden, ks)
CELLS = [(8, 32, 5), (24, 96, 5), (64, 128, 5), (128, 64, 5), (16, 96, 3), (64, 64, 3), (32, 32, 1), (64, 128, 1)]
CELLS_BF16 = [(16, 32, 5), (64, 64, 5)]
CELLS_REFUSED = [(8, 32, 3), (8, 32, 1)]    # cin = 40: 3x3 and 1x1 need cin % 16 == 0

# ---- F: dynamics stacks (channels, n_layers, units).  hip_ops.convstack_forward evaluates f once through enqueue_f, whose one-launch
# form (csrc/persist.hip) takes 64-channel stacks and 64 / 128 ones without a 128 -> 128 adjacency; each of these has a 32-, 96- or
# 256-channel side or that adjacency, so every layer goes through launch_conv on its own.  None is dropped: the trajectory tests build
# 64 / 64, 128 / 64 and (Tanh encoder fixture) 32 / 32 stacks only, so no other test pins a 32 <-> 96, 64 <-> 32, 128 -> 128 or
# 32 <-> 256 layer, or a 96 -> 96 / 256 -> .. one behind a declined Winograd image
STACKS = [(32, 2, 96), (64, 2, 32), (128, 2, 128), (32, 1, 256)]


def case_id(c):
    return "-".join(str(int(v)) if isinstance(v, bool) else str(v) for v in c)


def _seed(*key):
    return zlib.crc32(repr(key).encode()) & 0x7FFFFFF


@functools.lru_cache(maxsize=None)
def layer_values(b, cin, cout, ks, with_bias=True):
    """(x, w, bias): procedural, shared by every test that names the same layer."""
    s = _seed(b, cin, cout, ks)
    bound = 1.0 / float(cin * ks * ks) ** 0.5
    x = procedural_tensor((b, cin, 16, 16), s, -1.0, 1.0)
    w = procedural_tensor((cout, cin, ks, ks), s + 1, -bound, bound)
    bias = procedural_tensor((cout,), s + 2, -1.0, 1.0) if with_bias else None
    return x, w, bias


def _conv(x, w, bias, ks, relu):
    y = F.conv2d(x, w, bias, padding=ks // 2)
    return torch.relu(y) if relu else y


@functools.lru_cache(maxsize=None)
def layer_reference(case, bf16=False):
    """(float64 reference, d32) of a layer case; bf16: x and w rounded to bf16 first, the bias as it is."""
    b, cin1, cin2, cout, ks, relu, with_bias = case
    x, w, bias = layer_values(b, cin1 + cin2, cout, ks, with_bias)
    if bf16:
        x, w = x.bfloat16().float(), w.bfloat16().float()
    ref64 = _conv(x.double(), w.double(), None if bias is None else bias.double(), ks, relu)
    ref32 = _conv(x, w, bias, ks, relu)
    return ref64, rel_l2(ref32, ref64)


@functools.lru_cache(maxsize=None)
def dgrad_reference(b, cin, cout, ks):
    """Input gradient of a (cin -> cout) layer under a procedural output gradient: (w, gy, float64 autograd gradient, d32)."""
    x, w, _ = layer_values(b, cin, cout, ks)
    gy = procedural_tensor((b, cout, 16, 16), _seed("gy", b, cin, cout, ks), -1.0, 1.0)
    out = []
    for dt in (torch.float64, torch.float32):
        xr = x.to(dt).requires_grad_(True)
        F.conv2d(xr, w.to(dt), None, padding=ks // 2).backward(gy.to(dt))
        out.append(xr.grad)
    return w, gy, out[0], rel_l2(out[1], out[0])


def cell_values(i, h, ks, b=2):
    import _convgru_ref as ref
    s = _seed("cell", i, h, ks)
    return (ref.cell_state_dict(i, h, s % 1000, ks), procedural_tensor((b, i, 16, 16), s + 1, -1.0, 1.0),
            procedural_tensor((b, h, 16, 16), s + 2, -0.8, 0.8))


@functools.lru_cache(maxsize=None)
def cell_reference(i, h, ks):
    """(float32, float64) states after one step of oracle.reference_modules.convgru_cell."""
    import _convgru_ref as ref
    from oracle import reference_modules as rm
    sd, x, h0 = cell_values(i, h, ks)
    with torch.no_grad():
        return rm.convgru_cell(x, h0, sd), rm.convgru_cell(x.double(), h0.double(), ref.cast(sd, torch.float64))


def stack_values(ch, n_layers, units, b=3):
    """(state_dict, y): procedural weights within +-1/sqrt(fan_in) and biases of the default range, inputs in [-1, 1)."""
    import ode_rl_amd
    from conftest import procedural_state_dict
    s = _seed("stack", ch, n_layers, units)
    shapes = ode_rl_amd.ODEFunc(ch, ch, n_layers, units, False, "relu", final_act=False).state_dict()
    return procedural_state_dict(shapes, s % 1000), procedural_tensor((b, ch, 16, 16), s + 1, -1.0, 1.0)


@functools.lru_cache(maxsize=None)
def stack_reference(ch, n_layers, units):
    from oracle import reference_modules as rm
    sd, y = stack_values(ch, n_layers, units)
    ws, bs = rm.split_convnet_state(sd, "gradient_net.")
    with torch.no_grad():
        return rm.convnet_forward(y, ws, bs), rm.convnet_forward(y.double(), [w.double() for w in ws], [b.double() for b in bs])
