"""float64 reference formulas and input builders that more than one test file uses.  The comparisons are in tests/op_gate.py."""
import functools
import math

import torch
import torch.nn.functional as F

from oracle import raft_oracle as O


# ---------------------------------------------------------------------------------------------------------------------
# the ConvNeXt block's backward formulas of include/pfk.h (tests/test_sea_train_cpu.py holds them against autograd)
# ---------------------------------------------------------------------------------------------------------------------
def layernorm_bwd_ref(xhat, rstd, gamma, dy):
    """(b): rows [M, C]"""
    g = dy * gamma
    du = rstd[:, None] * (g - g.mean(1, keepdim=True) - xhat * (g * xhat).mean(1, keepdim=True))
    return du, (dy * xhat).sum(0), dy.sum(0)


def dwconv_bwd_ref(x, du, w, B, H, W):
    """(c): rows [M, C], w [C, k, k]; shifts written out tap by tap, zero outside the image, never across images"""
    C, k = w.shape[0], w.shape[-1]
    R = k // 2
    xi, di = x.view(B, H, W, C), du.view(B, H, W, C)
    xp, dp = F.pad(xi, (0, 0, R, R, R, R)), F.pad(di, (0, 0, R, R, R, R))
    dx = torch.zeros_like(xi)
    dw = torch.zeros_like(w)
    for ky in range(k):
        for kx in range(k):
            # du[(y - ky + R, x - kx + R)] = dp[y - ky + 2R, x - kx + 2R];  in[(y + ky - R, x + kx - R)] = xp[y + ky, x + kx]
            dx = dx + w[:, ky, kx] * dp[:, 2 * R - ky:2 * R - ky + H, 2 * R - kx:2 * R - kx + W]
            dw[:, ky, kx] = (di * xp[:, ky:ky + H, kx:kx + W]).sum((0, 1, 2))
    return dx.reshape(-1, C), dw, du.sum(0)


def gelu_bwd_ref(x, dy):
    """(d)"""
    return dy * (0.5 * (1 + torch.erf(x / math.sqrt(2))) + x * torch.exp(-x * x / 2) / math.sqrt(2 * math.pi))


# ---------------------------------------------------------------------------------------------------------------------
# the ConvGRU gate epilogues, restated on what a launch consumed
# ---------------------------------------------------------------------------------------------------------------------
def conv64(srcs, reals, weight, bias, res, b, h, w, kh, kw):
    """fp64 'same' convolution of pixel-major rows: cat(src[:, :real]) x weight [cout, sum(reals), kh, kw] + bias + res, [M, cout]"""
    x = torch.cat([s.cpu()[:, :r].double() for s, r in zip(srcs, reals)], 1)
    x = x.reshape(b, h, w, -1).permute(0, 3, 1, 2)
    v = F.conv2d(x, weight.double(), padding=(kh // 2, kw // 2)).permute(0, 2, 3, 1).reshape(b * h * w, -1)
    if bias is not None:
        v = v + bias.double().cpu()
    if res is not None:
        v = v + res.double().cpu()
    return v


def ref_zr(srcs, reals, weight, bias, res, h_rows, shape, k):
    """z = sigmoid(v[:, :Ch]), r*h = sigmoid(v[:, Ch:]) * h, v = conv + bias + residual (K8b: h is the bf16 twin)"""
    v = conv64(srcs, reals, weight, bias, res, *shape, *k)
    Ch = v.shape[1] // 2
    return torch.sigmoid(v[:, :Ch]), torch.sigmoid(v[:, Ch:]) * h_rows.double().cpu()


def ref_q(srcs, reals, weight, bias, res, z_rows, h_rows, shape, k):
    """h' = (1 - z) h + z tanh(conv + bias + residual), on the z the z|r launch stored and the fp32 h"""
    v = conv64(srcs, reals, weight, bias, res, *shape, *k)
    z, h = z_rows.double().cpu(), h_rows.double().cpu()
    return (1 - z) * h + z * torch.tanh(v)


# ---------------------------------------------------------------------------------------------------------------------
# input builders
# ---------------------------------------------------------------------------------------------------------------------
def coords_cases(B, h, w):
    """(name, [B, 2, h, w] lookup coordinates): integer, fractional, half-pixel, far outside, on the edges, non-finite"""
    g = torch.Generator().manual_seed(7)
    c0 = O.coords_grid(B, h, w)
    yield "integer", c0
    yield "fractional", c0 + torch.rand(B, 2, h, w, generator=g) * 16 - 8
    yield "half", c0 + 0.5
    yield "out_of_bounds", c0 + torch.randn(B, 2, h, w, generator=g) * 80
    edge = c0.clone()
    edge[:, 0] = torch.where(edge[:, 0] < w / 2, -0.25, w - 0.75)
    edge[:, 1] = torch.where(edge[:, 1] < h / 2, -1.0, float(h - 1))
    yield "edges", edge
    bad = c0.clone()
    bad[:, 0, 0, 0] = float("nan")
    bad[:, 1, 0, 1] = float("inf")
    bad[:, 0, 1, 0] = -float("inf")
    bad[:, 0, 1, 1] = 3.0e9
    bad[:, 1, 1, 2] = -2.5e7
    yield "nonfinite", bad


@functools.lru_cache(maxsize=None)
def convex_case(B, H, W, logit_scale):
    """fp32 inputs of the convex-upsampling backward, its float64 gradients and their sums of magnitudes; once per case"""
    g = torch.Generator().manual_seed(B * 100 + H * 10 + W + int(logit_scale))
    flow = torch.randn(B, 2, H, W, generator=g) * 3
    mask = torch.randn(B, 576, H, W, generator=g) * logit_scale
    go = torch.randn(B, 2, 8 * H, 8 * W, generator=g)
    f64, m64, g64 = flow.double().requires_grad_(), mask.double().requires_grad_(), go.double()
    out = O.convex_upsample(f64, m64)
    gflow, gmask = torch.autograd.grad((out * g64).sum(), (f64, m64), retain_graph=True)
    (gflow_mag,) = torch.autograd.grad((out * g64.abs()).sum(), f64)        # the softmax weights are >= 0: sum of 8 w |g|
    # magnitudes of dmask[k] = w_k (dw_k - sum_j w_j dw_j), dw_k = g_x v_x,k + g_y v_y,k
    with torch.no_grad():
        m = m64.view(B, 1, 9, 8, 8, H, W)
        wgt = torch.softmax(m, dim=2)[:, 0]                                                          # [B, 9, 8, 8, H, W]
        spread = (m.amax(2) - m.amin(2))[:, 0]                                                       # [B, 8, 8, H, W]
        up = F.unfold(8 * f64, [3, 3], padding=1).view(B, 2, 9, 1, 1, H, W).abs()
        gsub = g64.view(B, 2, H, 8, W, 8).permute(0, 1, 3, 5, 2, 4).abs()                            # [B, 2, sy, sx, H, W]
        T = (gsub[:, :, None] * up).sum(1)                                                           # [B, 9, 8, 8, H, W]
        gmask_mag = wgt * (T + (wgt * T).sum(1, keepdim=True))
    pm = lambda t: t.reshape(B, 576, H, W).permute(0, 2, 3, 1).reshape(B * H * W, 576)
    # K: a softmax weight is off by at most (2 spread + 19) units of 2^-24 relative — the rounded differences m_k - max in the
    # numerator and in the denominator (spread each), expf within 2 ulp twice (4 + 4), nine additions, the reciprocal, the product;
    # dmask then has its weight, dw_k (3 roundings), the dot (each term a weight, a dw, a product; nine additions), the subtraction
    # and the last product: at most 2 (2 spread + 19) + 15 on the magnitudes above.
    k_w = 2 * spread + 19
    k_mask = pm((2 * k_w + 15)[:, None].expand(B, 9, 8, 8, H, W))
    return {"flow": flow, "mask": mask, "go": go, "gflow": gflow, "gflow_mag": gflow_mag, "gmask": pm(gmask), "gmask_mag": pm(gmask_mag),
            "k_mask": k_mask, "k_flow": 9 * 64 + float(k_w.max()) + 2}


# ---------------------------------------------------------------------------------------------------------------------
# the LINEAR epilogue of pfk_conv2d_f32 / pfk_conv2d_group_f32 and the all-pairs correlation volumes, restated on what a launch consumes
# ---------------------------------------------------------------------------------------------------------------------
GRID = (2, 11, 13)          # M = 286 = 4 * 64 + 30 = 2 * 128 + 30; the image boundary (pixel 143) falls inside a tile
GRID_S2 = (3, 13, 15)       # stride 2: Ho x Wo = 7 x 8, M = 168 = 128 + 40
GRID_WIDE = (2, 7, 11)      # M = 154

# name: grid, (kh, kw), stride, sources [(real channels, view width)], cout, activation, scale, bias, residual, relu2
LINEAR_CASES = {
    # the cases of tests/test_gpu_linear_schedules.py that run on every schedule
    "motion":      (GRID, (3, 3), 1, [(64, 64), (146, 148), (2, 4)], 126, "relu", 1.0, True, False, False),
    "mask_head":   (GRID, (1, 1), 1, [(256, 256)], 576, "none", 0.25, True, False, False),
    "res_block":   (GRID, (3, 3), 1, [(96, 96)], 96, "relu", 1.0, True, True, True),
    "down_s2":     (GRID_S2, (3, 3), 2, [(64, 64)], 96, "relu", 1.0, True, True, True),
    "down_1x1_s2": (GRID_S2, (1, 1), 2, [(64, 64)], 96, "none", 1.0, True, False, False),
    "sep_1x5":     (GRID, (1, 5), 1, [(128, 128), (128, 128)], 128, "none", 1.0, True, False, False),
    "sep_5x1":     (GRID, (5, 1), 1, [(128, 128), (128, 128)], 128, "none", 1.0, False, False, False),
    "k7":          (GRID, (7, 7), 1, [(3, 4)], 40, "relu", 1.0, True, False, False),
    "convc1":      (GRID, (1, 1), 1, [(324, 324)], 256, "relu", 1.0, True, False, False),          # the last chunk holds 4 channels
    "res_scaled":  (GRID, (3, 3), 1, [(48, 48)], 72, "relu", 0.37, True, True, False),             # a residual AND a scale != 1
    "motion_res":  (GRID, (3, 3), 1, [(64, 64), (146, 148), (2, 4)], 126, "relu", 1.0, True, True, False),   # the alignment fall-backs
    "gelu_motion": (GRID, (3, 3), 1, [(64, 64), (146, 148), (2, 4)], 126, "gelu", 1.0, True, False, False),
    "gelu_res":    (GRID, (3, 3), 1, [(96, 96)], 96, "gelu", 0.5, True, True, False),
    "active":      (GRID, (3, 3), 1, [(128, 128)], 128, "relu", 1.0, True, False, False),          # cout_active 64 / cout_split 64
    # the problems of the grouped launches
    "g_c1":        (GRID, (1, 1), 1, [(324, 324)], 256, "relu", 1.0, True, True, False),
    "g_k3":        (GRID, (3, 3), 1, [(64, 64)], 96, "relu", 0.5, True, True, False),
    "g_mask":      (GRID, (1, 1), 1, [(256, 256)], 576, "none", 0.25, False, True, False),
    "g_sw0":       (GRID, (1, 1), 1, [(32, 32)], 4990, "relu", 1.0, True, True, False),
    "g_sw1":       (GRID, (1, 1), 1, [(36, 36)], 4992, "none", 0.5, True, True, False),
    "g_wide0":     (GRID_WIDE, (1, 1), 1, [(2048, 2048)], 128, "none", 0.37, False, True, False),
    "g_wide1":     (GRID_WIDE, (1, 1), 1, [(2080, 2080)], 256, "relu", 1.0, True, True, False),
}


def conv_out_hw(H, W, stride):
    """the output grid of a 'same'-padded convolution of stride `stride`"""
    return (H - 1) // stride + 1, (W - 1) // stride + 1


def _rows_of(t):
    """NCHW -> pixel-major [B * H * W, C]"""
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


def _images_of(rows, B, H, W):
    return rows.reshape(B, H, W, -1).permute(0, 3, 1, 2)


def linear_act64(pre, act):
    if act == "relu":
        return pre.clamp_min(0)
    if act == "gelu":
        return 0.5 * pre * (1 + torch.erf(pre / math.sqrt(2)))
    return pre


@functools.lru_cache(maxsize=None)
def linear_case(name):
    """One LINEAR launch, once per case: fp32 inputs exactly as the launch consumes them — `xs` [M_in, view width] rows per source
    (columns past `real` hold finite garbage: they meet zero weights), the conv weight `w` over the real channels, its packed form and
    `segs`, `bias`, `residual` [M_out, cout], `scale` (the float32 value, widened) — and in float64
        ref = relu2?( residual + scale * act(sum x w + bias) )        mag = |scale| (sum |x| |w| + |bias|) + |residual|
    with `pre` = sum x w + bias.  k = n + 4, n = kh kw sum(real) + [bias]: n roundings of the running sum in any order (stream-K
    partials included), one for the scale, one for the residual add, two to spare; relu is 1-Lipschitz."""
    from ptlflow_amd.packing import pack_conv_weight
    (B, H, W), (kh, kw), stride, sources, cout, act, scale, with_bias, with_res, relu2 = LINEAR_CASES[name]
    g = torch.Generator().manual_seed(sum(map(ord, name)) * 31 + cout)
    rnd = lambda *s: torch.randn(*s, generator=g)      # noqa: E731
    Ho, Wo = conv_out_hw(H, W, stride)
    M_in, M_out = B * H * W, B * Ho * Wo
    xs = [rnd(M_in, width) for _, width in sources]
    cin = sum(real for real, _ in sources)
    w = rnd(cout, cin, kh, kw) / math.sqrt(cin * kh * kw)
    bias = rnd(cout) * 0.3 if with_bias else None
    residual = rnd(M_out, cout) if with_res else None
    scale32 = float(torch.tensor(scale, dtype=torch.float32))
    segs, first = [], 0
    for real, width in sources:
        segs.append((first, real, width))
        first += real
    x64 = _images_of(torch.cat([x[:, :real].double() for x, (real, _) in zip(xs, sources)], 1), B, H, W)
    pad = (kh // 2, kw // 2)
    pre = _rows_of(F.conv2d(x64, w.double(), None, stride=stride, padding=pad))
    mag = _rows_of(F.conv2d(x64.abs(), w.double().abs(), None, stride=stride, padding=pad))
    if with_bias:
        pre, mag = pre + bias.double(), mag + bias.double().abs()
    ref, mag = scale32 * linear_act64(pre, act), abs(scale32) * mag
    if with_res:
        ref, mag = residual.double() + ref, mag + residual.double().abs()
    if relu2:
        ref = ref.clamp_min(0)
    n = kh * kw * cin + int(with_bias)
    return {"name": name, "grid": (B, H, W), "out_grid": (B, Ho, Wo), "k": (kh, kw), "stride": stride, "sources": sources, "reals": [r for r, _ in sources],
            "cout": cout, "act": act, "relu": act == "relu", "scale": scale32, "relu2": relu2, "M_in": M_in, "M": M_out,
            "xs": xs, "w": w, "segs": segs, "packed": pack_conv_weight(w, segs), "bias": bias, "residual": residual,
            "pre": pre, "ref": ref, "mag": mag, "K": n + 4, "steps": sum(kh * kw * ((width + 31) // 32) for _, width in sources)}


def linear_torch32(c):
    """torch's own fp32 CPU arithmetic of the same op: [M_out, cout]"""
    B, H, W = c["grid"]
    x = _images_of(torch.cat([x[:, :real] for x, real in zip(c["xs"], c["reals"])], 1), B, H, W)
    v = _rows_of(F.conv2d(x, c["w"], c["bias"], stride=c["stride"], padding=(c["k"][0] // 2, c["k"][1] // 2)))
    v = F.relu(v) if c["act"] == "relu" else F.gelu(v) if c["act"] == "gelu" else v
    v = v * c["scale"]
    if c["residual"] is not None:
        v = c["residual"] + v
    return F.relu(v) if c["relu2"] else v


# (B, N1, N2, D) of tests/test_gpu_volume_gate.py
VOLUMES_F32 = [(2, 117, 130, 64), (2, 132, 120, 128), (1, 2050, 2114, 32), (2, 2050, 4000, 32), (2, 150, 140, 36)]
VOLUMES_B16 = [(2, 130, 117, 40), (2, 132, 132, 64), (1, 257, 264, 72), (1, 40, 9, 8), (1, 4100, 4230, 8), (2, 70, 133, 40)]


@functools.lru_cache(maxsize=2)
def volume_case(B, N1, N2, D, dtype):
    """The all-pairs correlation out[b, i, j] = scale * <a[b, i], b[b, j]> on fp32 or bf16 rows: `a` [B, N1, D], `b` [B, N2, D] in
    `dtype`, scale = float32(1 / sqrt(D)), and in float64 ref = scale * sum a b, mag = |scale| sum |a| |b|; K = D + 3 (D roundings
    of the sum in any order, one for the scale, two to spare; bf16 x bf16 products are exact in fp32)."""
    g = torch.Generator().manual_seed(B * 1009 + N1 * 31 + N2 * 7 + D)
    a, b = torch.randn(B, N1, D, generator=g).to(dtype), torch.randn(B, N2, D, generator=g).to(dtype)
    scale = float(torch.tensor(1.0 / math.sqrt(D), dtype=torch.float32))
    a64, b64 = a.double(), b.double()
    return {"a": a, "b": b, "scale": scale, "K": D + 3, "ref": scale * torch.bmm(a64, b64.transpose(1, 2)),
            "mag": abs(scale) * torch.bmm(a64.abs(), b64.abs().transpose(1, 2))}


def volume_torch32(c, d=None):
    """torch's fp32 CPU arithmetic of the volume over the first `d` channels (default: all), rounded to the inputs' dtype"""
    a, b = c["a"][..., :d].float(), c["b"][..., :d].float()
    return (torch.bmm(a, b.transpose(1, 2)) * c["scale"]).to(c["a"].dtype)


# ---------------------------------------------------------------------------------------------------------------------
# the refinement loop's small direct kernels (pfk_misc.hip, the forward of pfk_upsample.hip), restated on what a launch consumes
# ---------------------------------------------------------------------------------------------------------------------
CIN2_GRIDS = [(2, 3, 21), (1, 1, 1), (2, 9, 33)]                 # shorter than the 7x7 halo with a 5-pixel last tile; one pixel; two images
CIN2_MFMA_GRIDS = CIN2_GRIDS + [(1, 5, 33), (2, 5, 4163)]        # 2 x 2 tiles with one-row / one-column tails; 524 tiles > the 512-block grid
FLOW_DELTA_GRIDS4 = [(2, 2, 5), (2, 1, 3), (1, 3, 9)]            # the 4-pixel kernel
FLOW_DELTA_GRIDS8 = [(2, 1024, 9), (4, 1024, 5)]                 # the 8-pixel kernel: B H ceil(W / 8) = 4096
UP_GRIDS = [(1, 1, 1), (2, 1, 5), (1, 6, 1), (2, 5, 7)]
UP_SCALES = [1.0, 40.0, 60.0]
UPFLOW_GRIDS = [(1, 1, 1), (1, 1, 5), (2, 6, 1), (2, 9, 13)]
LAYOUT_SHAPES = [(2, 33, 3, 11), (1, 1, 1, 1), (2, 126, 7, 45)]
SOFTMAX_COLS = [1, 5, 140, 257, 713]
SOFTMAX_ROWS = 7


def taps64(x, w, k):
    """'same' k x k convolution written tap by tap: x [B, H, W, cin], w [k * k, cin, cout] (tap-major), zero outside the image and
    never across images -> [B, H, W, cout], in x's dtype.  A NaN in x reaches exactly the outputs whose window covers it."""
    B, H, W, _ = x.shape
    R = k // 2
    xp = F.pad(x, (0, 0, R, R, R, R))
    out = torch.zeros(B, H, W, w.shape[2], dtype=x.dtype)
    for ky in range(k):
        for kx in range(k):
            out = out + xp[:, ky:ky + H, kx:kx + W] @ w[ky * k + kx]
    return out


def window_mask(B, H, W, b, y, x, R):
    """[B, H, W] bool: the pixels of image b whose (2R + 1)^2 window covers (y, x)"""
    m = torch.zeros(B, H, W, dtype=torch.bool)
    m[b, max(0, y - R):y + R + 1, max(0, x - R):x + R + 1] = True
    return m


@functools.lru_cache(maxsize=None)
def cin2_case(B, H, W, k, cout, relu=True, with_bias=True, nan_at=None):
    """pfk_conv_cin2: `rows` [M, 2] fp32 flow, the packed weight [k * k, 2, cout] and `bias` as the launch consumes them, and in float64,
    by a tap loop over the packed weight,  ref = relu?(bias + sum x w),  mag = |bias| + sum |x| |w|,  K = 2 k k + 2 (n = 2 k k products
    in any order; relu is 1-Lipschitz and keeps an exact zero where mag is 0).  `nan_at` = (y, x): the y component of that flow pixel of
    image 1 is NaN, `nan` [M, cout] the outputs whose window covers it (ref and mag are NaN there and only there)."""
    from ptlflow_amd.packing import pack_cin2_weight
    g = torch.Generator().manual_seed(((B * 131 + H) * 131 + W) * 131 + k * 17 + cout)
    flow = torch.randn(B, 2, H, W, generator=g) * 3
    w = torch.randn(cout, 2, k, k, generator=g) / k
    bias = torch.randn(cout, generator=g) * 0.3 if with_bias else None
    nan = torch.zeros(B, H, W, dtype=torch.bool)
    if nan_at is not None:
        flow[1, 1, nan_at[0], nan_at[1]] = float("nan")
        nan = window_mask(B, H, W, 1, *nan_at, k // 2)
    packed = pack_cin2_weight(w)
    x64, w64 = flow.double().permute(0, 2, 3, 1), packed.double()
    pre, mag = taps64(x64, w64, k), taps64(x64.abs(), w64.abs(), k)
    if with_bias:
        pre, mag = pre + bias.double(), mag + bias.double().abs()
    ref = pre.clamp_min(0) if relu else pre
    M = B * H * W
    return {"grid": (B, H, W), "k": k, "cout": cout, "relu": relu, "flow": flow, "rows": _rows_of(flow).contiguous(), "w": w, "packed": packed,
            "bias": bias, "ref": ref.reshape(M, cout), "mag": mag.reshape(M, cout), "K": 2 * k * k + 2,
            "nan": nan.reshape(M, 1).expand(M, cout).clone()}


def cin2_torch32(c, flow=None, w=None):
    """torch's fp32 CPU convolution of the same op: [M, cout]"""
    v = F.conv2d(c["flow"] if flow is None else flow, c["w"] if w is None else w, c["bias"], padding=c["k"] // 2)
    return _rows_of(F.relu(v) if c["relu"] else v)


@functools.lru_cache(maxsize=None)
def flow_delta_case(B, H, W, cin, dtype=torch.float32, nan_corners=False):
    """pfk_flow_delta: `x` [M, cin] rows in `dtype`, FlowHead.conv2's weight `w` [2, cin, 3, 3], its packed form [9, 2, cin], `bias` [2],
    `c0` / `c1` [B, 2, H, W], and in float64 on the widened rows  delta = bias + sum x w,  mag = |bias| + sum |x| |w|  [B, 2, H, W],
    K = 9 cin + 2.  `nan_corners`: the input rows of the four corner pixels of image 1 are NaN; `nan` marks their 3x3 neighbours in
    image 1 — were the row above y = 0 of image 1 image 0's last row, image 0's last row would be NaN too."""
    from ptlflow_amd.packing import pack_flow_head_weight
    g = torch.Generator().manual_seed(((B * 131 + H) * 131 + W) * 131 + cin)
    M = B * H * W
    x = torch.randn(M, cin, generator=g).to(dtype)
    w = torch.randn(2, cin, 3, 3, generator=g) / math.sqrt(9 * cin)
    bias = torch.randn(2, generator=g) * 0.3
    c0 = O.coords_grid(B, H, W)
    c1 = c0 + torch.randn(B, 2, H, W, generator=g) * 2
    nan = torch.zeros(B, H, W, dtype=torch.bool)
    if nan_corners:
        img = x.view(B, H, W, cin)
        for y in (0, H - 1):
            for xx in (0, W - 1):
                img[1, y, xx] = float("nan")
                nan |= window_mask(B, H, W, 1, y, xx, 1)
    packed = pack_flow_head_weight(w)
    x64, w64 = x.double().view(B, H, W, cin), packed.double().transpose(1, 2)          # [9, cin, 2]
    b64 = bias.double().view(1, 2, 1, 1)
    ref = taps64(x64, w64, 3).permute(0, 3, 1, 2) + b64
    mag = taps64(x64.abs(), w64.abs(), 3).permute(0, 3, 1, 2) + b64.abs()
    return {"grid": (B, H, W), "cin": cin, "x": x, "w": w, "packed": packed, "bias": bias, "c0": c0, "c1": c1, "ref": ref, "mag": mag,
            "K": 9 * cin + 2, "nan": nan[:, None].expand(B, 2, H, W).clone()}


def flow_delta_torch32(c, x=None):
    """torch's fp32 CPU convolution on the widened rows: [B, 2, H, W]"""
    B, H, W = c["grid"]
    x = c["x"].float() if x is None else x
    return F.conv2d(_images_of(x, B, H, W), c["w"][:, :x.shape[1]], c["bias"], padding=1)


def convex_fwd64(flow, mask, info=None):
    """The forward x8 convex upsampling in float64 on the fp32 values a launch reads: flow [B, 2, H, W], mask [B, 576, H, W] (bf16
    logits widened), info [B, n, H, W] or None ->  ref, mag, k  [B, 2 + n, 8H, 8W]  with
        w_k = softmax_k(mask[k, sy, sx]),   ref = sum_k w_k v_k,   mag = sum_k w_k |v_k|,   v = 8 flow (exact) or info, zero outside
    the image.  k = k_w + 11 per element: k_w = 2 spread + 19 is the relative error of a weight in units of 2^-24 (`convex_case`'s
    comment; spread = max - min of the nine logits, over the finite ones: expf(-inf) is an exact 0), and the combination adds one
    rounding for each product and nine additions, one to spare."""
    B, _, H, W = flow.shape
    m = mask.double().view(B, 1, 9, 8, 8, H, W)
    wgt = torch.softmax(m, dim=2)
    top = m.amax(2, keepdim=True)
    spread = (top - torch.where(torch.isinf(m), top, m).amin(2, keepdim=True))[:, :, 0]               # [B, 1, 8, 8, H, W]
    v = 8 * flow.double() if info is None else torch.cat([8 * flow.double(), info.double()], 1)
    C = v.shape[1]
    nb = F.unfold(v, [3, 3], padding=1).view(B, C, 9, 1, 1, H, W)
    up = lambda t: t.permute(0, 1, 4, 2, 5, 3).reshape(B, C, 8 * H, 8 * W)        # noqa: E731   [B, C, sy, sx, H, W] -> [B, C, 8H, 8W]
    return up((wgt * nb).sum(2)), up((wgt * nb.abs()).sum(2)), up((2 * spread + 30).expand(B, C, 8, 8, H, W))


@functools.lru_cache(maxsize=None)
def convex_fwd_case(B, H, W, logit_scale, b16=False, zero_image=None):
    """fp32 `flow` [B, 2, H, W], `info` [B, 8, H, W] (a launch with n_info channels reads the first n) and `mask` [B, 576, H, W] logits
    (`b16`: bf16), with `convex_fwd64` of them (channels 0, 1 the flow, 2.. the info); `zero_image`: that image's flow is zero"""
    g = torch.Generator().manual_seed(B * 1000 + H * 100 + W * 10 + int(logit_scale) + 5)
    flow = torch.randn(B, 2, H, W, generator=g) * 3
    info = torch.randn(B, 8, H, W, generator=g)
    mask = torch.randn(B, 576, H, W, generator=g) * logit_scale
    if b16:
        mask = mask.to(torch.bfloat16)
    if zero_image is not None:
        flow[zero_image] = 0.0
    ref, mag, k = convex_fwd64(flow, mask.float(), info)
    return {"grid": (B, H, W), "flow": flow, "info": info, "mask": mask, "ref": ref, "mag": mag, "k": k}


def upflow8_axis(n_in):
    """the kernel's index arithmetic along one axis, in fp32 as its comment gives it: (i0, i1, lambda1) for the 8 n_in outputs"""
    n_out = 8 * n_in
    scale = torch.tensor(float(n_in - 1), dtype=torch.float32) / torch.tensor(float(n_out - 1), dtype=torch.float32)
    src = scale * torch.arange(n_out, dtype=torch.float32)
    i0 = src.to(torch.int64)                                    # truncation; src >= 0
    lam1 = src - i0.to(torch.float32)
    i1 = i0 + (i0 < n_in - 1).to(torch.int64)
    return i0, i1, lam1


@functools.lru_cache(maxsize=None)
def upflow8_case(B, H, W):
    """pfk_upflow8: `c0`, `c1` [B, 2, H, W] and, with the fp32 indices and lambdas of `upflow8_axis`, the float64 blend of c1 - c0:
    ref = 8 sum ly lx v,  mag = 8 sum ly lx |v|  [B, 2, 8H, 8W];  K = 8: the difference, the two 1 - lambda, the four products in two
    levels and two additions are at most 7 roundings on the path of a term, and the factor 8 is exact."""
    g = torch.Generator().manual_seed(B * 100 + H * 10 + W)
    c0 = torch.randn(B, 2, H, W, generator=g) * 30
    c1 = c0 + torch.randn(B, 2, H, W, generator=g) * 4
    v = c1.double() - c0.double()
    y0, y1, ly = upflow8_axis(H)
    x0, x1, lx = upflow8_axis(W)
    ly, lx = ly.double()[:, None], lx.double()[None, :]
    ref, mag = 0.0, 0.0
    for yi, wy in ((y0, 1 - ly), (y1, ly)):
        for xi, wx in ((x0, 1 - lx), (x1, lx)):
            t = v[:, :, yi][:, :, :, xi]
            ref, mag = ref + wy * wx * t, mag + wy * wx * t.abs()
    return {"grid": (B, H, W), "c0": c0, "c1": c1, "ref": 8 * ref, "mag": 8 * mag, "K": 8}


@functools.lru_cache(maxsize=None)
def softmax_rows_case(cols, logit_scale):
    """pfk_softmax_rows: `x` [7, cols] fp32 logits (row 3 holds -inf in all but two columns where cols >= 3), p = softmax in float64 and
    k = 2 spread_row + cols + 19: the rounded differences x - max in the numerator and the denominator (spread each), expf twice, cols
    additions, the division (spread over the finite logits: expf(-inf) is an exact 0)"""
    g = torch.Generator().manual_seed(cols * 7 + int(logit_scale))
    x = torch.randn(SOFTMAX_ROWS, cols, generator=g) * logit_scale
    if cols >= 3:
        keep = torch.zeros(cols, dtype=torch.bool)
        keep[[1, cols - 1]] = True
        x[3, ~keep] = float("-inf")
    x64 = x.double()
    top = x64.amax(1, keepdim=True)
    spread = top - torch.where(torch.isinf(x64), top, x64).amin(1, keepdim=True)
    p = torch.softmax(x64, dim=1)
    return {"x": x, "ref": p, "mag": p, "k": (2 * spread + cols + 19).expand(SOFTMAX_ROWS, cols)}
