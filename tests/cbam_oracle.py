"""Plain float64 statement of every pass of csrc/cbam.hip (unet2.py:6-74), one function per kernel, NHWC as the kernels see
their operands: every input is taken as it is stored (already rounded to the storage dtype by the caller), evaluated in f64.

The three "first maximum" rules are written out as `where(mask, index, BIG).min()` -- never left to what torch.max returns:
  * arg-max over channels of o1 = ca * z            (spatial_stats: the first channel holding the maximum),
  * the global max-pool's pixel per (image, channel) (first: the first pixel, row-major, holding the extreme raw value),
  * the 2x2 max-pool's position                     (bwd1: the first of (0,0), (0,1), (1,0), (1,1) holding the window's maximum).
tests/test_cbam_host.py ties these to CPU torch autograd of the reference formulation; the GPU tests then need this file only.

Tie inputs (tie_case): every factor lies on a dyadic grid -- y, shift, mean and the incoming gradients are multiples of 1/4 in
[-1, 1], scale and invstd are powers of two (scale with both signs), ca in {1/4, 1/2}, sa in {1/4, 1/2, 3/4}, d_mean a multiple
of C / 4 and d_avgz a multiple of H W / 4 (the kernels divide them by C and H W) -- so that every product and every sum of the
passes is exact in f32 whatever the order, and every stored output has at most 8 significant bits (exact in bf16).  The values
come from integer arithmetic on the indices, not from a random generator: the tie counts asserted in the tests are the same
everywhere.  (Two planted channels per fourth pixel carry a y of up to 9 in steps of 1/2, z = 2 or 4, o1 = 1.)  Worst-case
widths (C = 512, 960 pixels): sum_c g * o1 < 2^17 steps of 1/128, du < 2^21 steps of 1/2048, the d_ca partials (|d_o1 z| <= 8)
< 2^20 steps of 1/128, a workgroup's BatchNorm rows (|d_z xhat| <= 33) < 2^21 steps of 1/64: all below the 2^24 of an f32
significand.
"""
import torch

BIG = 0x7FFFFFFF


def f64(t):
    return t.detach().double().cpu()


# ------------------------------------------------------------------ launch geometry that the tie counts refer to
def vec(bf16):
    return 8 if bf16 else 4


def lane_of_channel(C, bf16):
    """(lane, vector-of-the-lane) of every channel in the lanes-per-pixel kernels: a lane holds one 16-byte vector of channels,
    two (vector v and v + C/N/2) when there are more than 64 vectors (f32 with 512 channels)"""
    N = vec(bf16)
    ncv = C // N
    nvl = 2 if ncv > 64 else 1
    cpp = ncv // nvl
    v = torch.arange(C) // N
    return v % cpp, v // cpp


def group_grid(C, bf16, B, H, W):
    """(workgroups per image, pixels per workgroup pass) of abc_cbam_spatial_stats / abc_cbam_bwd1"""
    ncv = C // vec(bf16)
    cpp = ncv // 2 if ncv > 64 else ncv
    ppb = 256 // cpp
    b = (H * W + 4 * ppb - 1) // (4 * ppb)
    return max(1, min(b, max(1, 4096 // B))), ppb


# ------------------------------------------------------------------ the conv epilogue's four rows, synthesised
def chunk_sizes(HW, T):
    """T uneven pixel chunks (every one non-empty) that cover HW pixels"""
    assert 1 <= T <= HW
    w = torch.tensor([1 + (i * 7) % 5 for i in range(T)], dtype=torch.float64)
    cum = torch.floor((HW - T) * torch.cumsum(w, 0) / w.sum() + 1e-9).long()
    sizes = 1 + torch.diff(cum, prepend=torch.zeros(1, dtype=torch.long))
    assert int(sizes.sum()) == HW and int(sizes.min()) >= 1
    return sizes.tolist()


def conv_partials(y, T):
    """y [B,H,W,C] -> f32 [B*T][4][C]: (sum, sum of squares, max, min) of each of T pixel chunks per image"""
    B, H, W, C = y.shape
    yy = f64(y).reshape(B, H * W, C)
    rows = []
    for n in range(B):
        for ch in torch.split(yy[n], chunk_sizes(H * W, T), dim=0):
            rows.append(torch.stack([ch.sum(0), (ch * ch).sum(0), ch.max(0)[0], ch.min(0)[0]]))
    return torch.stack(rows).float()


# ------------------------------------------------------------------ forward
def first_extreme(y, scale):
    """ext[n][c]: the raw value whose BatchNorm image is max(z) (max of y for scale >= 0, min otherwise); first[n][c]: the first
    pixel (row-major) holding it"""
    B, H, W, C = y.shape
    yy = f64(y).reshape(B, H * W, C)
    ext = torch.where(f64(scale) >= 0, yy.max(1)[0], yy.min(1)[0])
    q = torch.arange(H * W).view(1, -1, 1).expand(B, H * W, C)
    first = torch.where(yy == ext[:, None, :], q, torch.full_like(q, BIG)).min(1)[0]
    return ext, first


def channel_fwd(y, scale, shift, w1, b1, w2, b2):
    """ChannelAttentionModule (unet2.py:6-22) on z = scale * y + shift"""
    B, H, W, C = y.shape
    sc, sh = f64(scale), f64(shift)
    ext, first = first_extreme(y, scale)
    avgz = sc * f64(y).reshape(B, H * W, C).mean(1) + sh
    maxz = sc * ext + sh
    w1, b1, w2, b2 = f64(w1), f64(b1), f64(w2), f64(b2)
    ha = torch.relu(avgz @ w1.t() + b1)
    hm = torch.relu(maxz @ w1.t() + b1)
    ca = torch.sigmoid(2 * b2 + (ha + hm) @ w2.t())
    return dict(avgz=avgz, maxz=maxz, ext=ext, first=first, hid_avg=ha, hid_max=hm, ca=ca)


def o1_of(y, scale, shift, ca):
    return f64(ca)[:, None, None, :] * (f64(y) * f64(scale) + f64(shift))


def spatial_stats(y, scale, shift, ca):
    """st[..., 0] = mean over channels of o1, st[..., 1] = max, amax = the FIRST channel holding the max"""
    o1 = o1_of(y, scale, shift, ca)
    C = o1.shape[-1]
    m = o1.max(-1)[0]
    c = torch.arange(C).expand_as(o1)
    amax = torch.where(o1 == m[..., None], c, torch.full_like(c, BIG)).min(-1)[0]
    return torch.stack([o1.sum(-1) / C, m], -1), amax


def pool2(t):
    """2x2 max-pool (floor) of [B,H,W,C] and the FIRST position (0..3 = (0,0), (0,1), (1,0), (1,1)) holding each maximum"""
    B, H, W, C = t.shape
    h2, w2 = H // 2, W // 2
    win = t[:, :2 * h2, :2 * w2].reshape(B, h2, 2, w2, 2, C).permute(0, 1, 3, 2, 4, 5).reshape(B, h2, w2, 4, C)
    m = win.max(3)[0]
    k = torch.arange(4).view(1, 1, 1, 4, 1).expand_as(win)
    arg = torch.where(win == m[:, :, :, None, :], k, torch.full_like(k, BIG)).min(3)[0]
    return m, arg


def apply_fwd(y, scale, shift, ca, sa, res, res_pool=False):
    """out = relu(sa * ca * z + r), r = res or its 2x2 max-pool"""
    r = f64(res)
    if res_pool:
        r = pool2(r)[0]
    return torch.relu(f64(sa)[..., None] * o1_of(y, scale, shift, ca) + r)


# ------------------------------------------------------------------ backward
def unpool(out, d_pool):
    """gradient of max_pool2d(out, 2) wrt out: the pooled gradient lands on the first maximum of its window; a last odd row /
    column lies in no window"""
    B, H, W, C = out.shape
    h2, w2 = H // 2, W // 2
    _, arg = pool2(f64(out))
    k = torch.arange(4).view(1, 1, 1, 4, 1)
    sel = (arg[:, :, :, None, :] == k).double() * f64(d_pool)[:, :, :, None, :]        # [B,h2,w2,4,C]
    g = torch.zeros(B, H, W, C, dtype=torch.float64)
    g[:, :2 * h2, :2 * w2] = sel.reshape(B, h2, w2, 2, 2, C).permute(0, 1, 3, 2, 4, 5).reshape(B, 2 * h2, 2 * w2, C)
    return g


def bwd1(y, scale, shift, ca, sa, out, d_same=None, d_pool=None):
    """g = (d_same + unpool(d_pool)) * [out > 0];  du = (sum_c g * o1) * sa * (1 - sa)"""
    o = f64(out)
    g = torch.zeros_like(o)
    if d_same is not None:
        g = g + f64(d_same)
    if d_pool is not None:
        g = g + unpool(out, d_pool)
    g = g * (o > 0)
    s = f64(sa)
    return g, (g * o1_of(y, scale, shift, ca)).sum(-1) * s * (1 - s)


def bwd2(y, scale, shift, g, sa, dst, amax):
    """d_o1 = g * sa + d_mean / C + [c == amax] * d_max;  d_ca[n][c] = sum over pixels of d_o1 * z"""
    z = f64(y) * f64(scale) + f64(shift)
    C = z.shape[-1]
    d = f64(dst)
    hit = (torch.arange(C).view(1, 1, 1, C) == amax.cpu().long()[..., None]).double()
    d_o1 = f64(g) * f64(sa)[..., None] + d[..., 0:1] / C + hit * d[..., 1:2]
    return d_o1, (d_o1 * z).sum((1, 2))


def channel_bwd(d_ca, ca, hid_avg, hid_max, avgz, maxz, w1, w2):
    """backward of ca = sigmoid(MLP(avgz) + MLP(maxz)) given d_ca (the pass-2 partials summed)"""
    ca, ha, hm, az, mz, w1, w2 = (f64(t) for t in (ca, hid_avg, hid_max, avgz, maxz, w1, w2))
    dt = f64(d_ca) * ca * (1 - ca)                      # [B][C]: d(pre-sigmoid)
    dh = dt @ w2                                        # [B][mid]
    dha, dhm = dh * (ha > 0), dh * (hm > 0)
    return dict(dw2=dt.t() @ (ha + hm), db2=2 * dt.sum(0), dw1=dha.t() @ az + dhm.t() @ mz, db1=(dha + dhm).sum(0),
                d_avgz=dha @ w1, d_maxz=dhm @ w1)


def bwd3(y, mean, invstd, d_o1, ca, d_avgz, d_maxz, first):
    """d_z = d_o1 * ca + d_avgz / HW + [pixel == first] * d_maxz;  rows (sum d_z, sum d_z * xhat) per channel"""
    B, H, W, C = y.shape
    q = torch.arange(H * W).view(1, H, W, 1)
    hit = (q == first.cpu().long()[:, None, None, :]).double()
    dz = f64(d_o1) * f64(ca)[:, None, None, :] + f64(d_avgz)[:, None, None, :] / (H * W) + hit * f64(d_maxz)[:, None, None, :]
    xhat = (f64(y) - f64(mean)) * f64(invstd)
    return dz, torch.stack([dz.sum((0, 1, 2)), (dz * xhat).sum((0, 1, 2))])


# ------------------------------------------------------------------ inputs full of exact ties
def _grid(B, H, W, C, a, b, c, m):
    n = torch.arange(B).view(B, 1, 1, 1)
    q = (torch.arange(H).view(1, H, 1, 1) * W + torch.arange(W).view(1, 1, W, 1))
    ch = torch.arange(C).view(1, 1, 1, C)
    return (n * a + q * b + ch * c + (q * ch) % 11 + (q // 3) * (ch // 5) + (q * q) % 7) % m


def tie_res(B, H, W, C):
    return (_grid(B, H, W, C, 5, 3, 11, 9) - 4).double() / 4


def tie_case(B, H, W, C):
    """a dict of f64 tensors on the dyadic grids of the module docstring (all exactly representable in bf16)"""
    k = _grid(B, H, W, C, 7, 13, 5, 9)
    t = {"y": (k - 4).double() / 4}
    ci = torch.arange(C)
    t["scale"] = torch.tensor([1.0, -0.5, 0.5, -1.0]).double()[(ci + ci // 4) % 4]
    t["shift"] = ((ci * 3 + ci // 8) % 3 - 1).double() / 2
    t["mean"] = ((ci * 5 + ci // 3) % 5 - 2).double() / 4
    t["invstd"] = torch.tensor([1.0, 2.0]).double()[(ci + ci // 2) % 2]
    bc = torch.arange(B).view(B, 1) * 3 + ci.view(1, C)
    t["ca"] = torch.tensor([0.5, 0.25]).double()[(bc + bc // 7) % 2]
    # every fourth pixel: two channels half the channel count apart (two lanes of the pixel's group; the two vectors of ONE lane where a
    # lane holds two) are raised to o1 = 1 exactly, above every other channel's o1 <= 3/4: y = (1 / ca - shift) / scale, |y| <= 9
    sel = torch.arange(0, H * W, 4)
    yv = t["y"].view(B, H * W, C)
    for half in (0, C // 2):
        cc = (sel // 4 * 37 + sel // 20 * 3) % (C // 2) + half
        yv[:, sel, cc] = (1 / t["ca"][:, cc] - t["shift"][cc]) / t["scale"][cc]
    q = _grid(B, H, W, 1, 3, 5, 0, 3)[..., 0]
    t["sa"] = (q + 1).double() / 4
    t["res"] = tie_res(B, H, W, C)
    # the block's output as stored: half of it ReLU zeros, and every fifth 2x2 window four equal positive values in every channel
    t["out"] = torch.relu((_grid(B, H, W, C, 11, 1, 3, 7) - 3).double() / 4)
    wy, wx = torch.arange(H).view(1, H, 1, 1) // 2, torch.arange(W).view(1, 1, W, 1) // 2
    t["out"] = torch.where(((wy * 3 + wx) % 5 == 0).expand_as(t["out"]), torch.full_like(t["out"], 0.75), t["out"])
    t["d_same"] = (_grid(B, H, W, C, 2, 11, 7, 9) - 4).double() / 4
    t["d_pool"] = (_grid(B, H // 2, W // 2, C, 9, 7, 3, 9) - 4).double() / 4
    t["g"] = t["d_same"] * (t["out"] > 0)
    d2 = _grid(B, H, W, 2, 4, 9, 1, 5) - 2
    t["dst"] = torch.stack([d2[..., 0].double() * C / 4, d2[..., 1].double() / 4], -1)      # (d_mean, d_max)
    t["d_o1"] = (_grid(B, H, W, C, 6, 17, 9, 9) - 4).double() / 4
    t["d_avgz"] = ((bc + bc // 5) % 5 - 2).double() * (H * W) / 4
    t["d_maxz"] = ((bc * 3 + bc // 4) % 7 - 3).double() / 4
    return t


def tie_counts(t, bf16):
    """how many exact ties the case holds where a kernel has to choose:
      lanes  : pixels whose channel maximum of o1 is held by channels of two different lanes of the pixel's lane group,
      vectors: pixels where it is held in both vectors of one lane (only where a lane has two: f32, 512 channels),
      groups : (image, channel) pairs whose extreme raw value is held by pixels of two different workgroups,
      window : (2x2 window, channel) pairs of `out` with four equal positive values"""
    B, H, W, C = t["y"].shape
    o1 = o1_of(t["y"], t["scale"], t["shift"], t["ca"])
    top = o1 == o1.max(-1, keepdim=True)[0]                            # [B,H,W,C]
    lane, v = lane_of_channel(C, bf16)
    nl = int(lane.max()) + 1
    lanes_hit = torch.zeros(B, H, W, nl).index_add_(3, lane, top.float()) > 0
    lanes = int((lanes_hit.sum(-1) > 1).sum())
    vectors = 0
    if int(v.max()) == 1:
        a = torch.zeros(B, H, W, nl).index_add_(3, lane[v == 0], top[..., v == 0].float()) > 0
        b = torch.zeros(B, H, W, nl).index_add_(3, lane[v == 1], top[..., v == 1].float()) > 0
        vectors = int((a & b).any(-1).sum())
    nwg, ppb = group_grid(C, bf16, B, H, W)
    ext, _ = first_extreme(t["y"], t["scale"])
    hold = (t["y"].reshape(B, H * W, C) == ext[:, None, :])
    wg = (torch.arange(H * W) // ppb) % nwg
    wg_hit = torch.zeros(B, nwg, C).index_add_(1, wg, hold.float()) > 0
    groups = int((wg_hit.sum(1) > 1).sum())
    m, _ = pool2(t["out"])
    h2, w2 = H // 2, W // 2
    win = t["out"][:, :2 * h2, :2 * w2].reshape(B, h2, 2, w2, 2, C)
    window = int(((win == m[:, :, None, :, None, :]).all(2).all(3) & (m > 0)).sum())
    return dict(lanes=lanes, vectors=vectors, groups=groups, window=window)
