"""ROIAlign / ROIPool / LevelMapper restated on the CPU from the reference's CUDA sources (csrc/cuda/ROIAlign_cuda.cu:15-254,
csrc/cuda/ROIPool_cuda.cu:16-108, modeling/poolers.py:11-42), independent of scan_amd.

Positions, grids, weights and cell indices are formed in fp32 operation by operation (numpy float32 arrays: every elementwise
operation is rounded on its own, in the source's left-to-right order).  Values and gradients are then computed in fp64 from
those fp32 weights, together with the sums of absolute terms the error bounds of tests/test_gpu_roi.py are relative to.

Layout: x is the row matrix [M, C] of a pyramid (level -> image -> y -> x), outputs are channel-last [K, PH, PW, C].
A ROI whose image index is outside [0, N) or whose level is outside the pyramid gives zeros, argmax -1 and no gradient."""
import numpy as np
import torch

f32 = np.float32
FLT_MAX = float(np.finfo(np.float32).max)

# the pyramid every ROI test uses: three levels, none a multiple of anything
N_IMAGES = 2
SIZES = ((13, 17), (7, 9), (4, 5))
SCALES = (0.25, 0.125, 0.0625)


def row_offsets(n, sizes):
    off = [0]
    for h, w in sizes:
        off.append(off[-1] + n * h * w)
    return off


# ----------------------------------------------------------------------------- LevelMapper
def level_mapper(boxes, k_min, k_max, s0=224, lvl0=4, eps=1e-6):
    """modeling/poolers.py:31-42 on an fp32 [K, 4] xyxy box tensor -> int64 levels"""
    boxes = boxes.float()
    area = (boxes[:, 2] - boxes[:, 0] + 1) * (boxes[:, 3] - boxes[:, 1] + 1)  # BoxList.area(), TO_REMOVE = 1
    s = torch.sqrt(area)
    lv = torch.floor(lvl0 + torch.log2(s / s0 + eps))
    lv = torch.clamp(lv, min=k_min, max=k_max)
    return lv.to(torch.int64) - int(k_min)


# ----------------------------------------------------------------------------- ROIAlign
def _place(roi, level, n_images, n_levels):
    n = int(roi[0])  # int roi_batch_ind = offset_bottom_rois[0]
    if not (0 <= n < n_images) or not (0 <= level < n_levels):
        return None
    return n


def _axis(start, binsz, P, g, size):
    """the P * g samples of one axis: fp32 position, live, low / high cell, l, h (ROIAlign_cuda.cu:109, :22-51)"""
    p = np.repeat(np.arange(P, dtype=np.int64), g).astype(f32)
    i = np.tile(np.arange(g, dtype=np.int64), P).astype(f32)
    y = (start + p * binsz) + ((i + f32(.5)) * binsz) / f32(g)
    pos = y.copy()
    live = ~((y < f32(-1.0)) | (y > f32(size)))
    y = np.where(y <= 0, f32(0), y).astype(f32)
    y = np.where(live, y, f32(0)).astype(f32)
    lo = y.astype(np.int64)
    top = lo >= size - 1
    lo = np.where(top, size - 1, lo)
    hi = np.where(top, size - 1, lo + 1)
    y = np.where(top, lo.astype(f32), y).astype(f32)
    l = (y - lo.astype(f32)).astype(f32)
    h = (f32(1.0) - l).astype(f32)
    return pos, live, lo, hi, l, h


def align_geometry(roi, scale, PH, PW, sr):
    """ROIAlign_cuda.cu:82-104 in fp32: start_h, start_w, bin_h, bin_w, g_h, g_w"""
    r = np.asarray(roi, dtype=f32)
    s = f32(scale)
    sw, sh, ew, eh = r[1] * s, r[2] * s, r[3] * s, r[4] * s
    rw = max(f32(ew - sw), f32(1.0))
    rh = max(f32(eh - sh), f32(1.0))
    bh, bw = f32(rh / f32(PH)), f32(rw / f32(PW))
    gh = sr if sr > 0 else int(np.ceil(f32(rh / f32(PH))))
    gw = sr if sr > 0 else int(np.ceil(f32(rw / f32(PW))))
    return sh, sw, bh, bw, gh, gw


def align_samples(roi, level, PH, PW, sr, n_images=N_IMAGES, sizes=SIZES, scales=SCALES):
    """None for a ROI outside the batch / pyramid, else a dict of fp32 / int arrays over [PH * g_h, PW * g_w]:
    pos_y [PH g_h], pos_x [PW g_w], live, w [4, ., .] (w1..w4), cell [4, ., .] (y * W + x of the level), g = (g_h, g_w)"""
    n = _place(roi, level, n_images, len(sizes))
    if n is None:
        return None
    H, W = sizes[level]
    sh, sw, bh, bw, gh, gw = align_geometry(roi, scales[level], PH, PW, sr)
    py, ly_, ylo, yhi, ly, hy = _axis(sh, bh, PH, gh, H)
    px, lx_, xlo, xhi, lx, hx = _axis(sw, bw, PW, gw, W)
    live = ly_[:, None] & lx_[None, :]
    w = np.stack([hy[:, None] * hx[None, :], hy[:, None] * lx[None, :], ly[:, None] * hx[None, :], ly[:, None] * lx[None, :]])
    cell = np.stack([ylo[:, None] * W + xlo[None, :], ylo[:, None] * W + xhi[None, :], yhi[:, None] * W + xlo[None, :],
                     yhi[:, None] * W + xhi[None, :]])
    w = np.where(live[None], w, f32(0)).astype(f32)
    cell = np.where(live[None], cell, -1)
    return dict(n=n, g=(gh, gw), pos_y=py, pos_x=px, live=live, w=w, cell=cell)


def roi_align(x, rois, levels, PH, PW, sr, n_images=N_IMAGES, sizes=SIZES, scales=SCALES):
    """x [M, C] (any float dtype, promoted to fp64), rois [K, 5], levels [K] -> dict:
    y [K, PH, PW, C] fp64, yabs = sum over samples and corners of |w v| / count (what the forward bound is relative to),
    terms [K] = g_h * g_w (0 for a ROI outside)"""
    x = x.double()
    K, C = len(rois), x.shape[1]
    off = row_offsets(n_images, sizes)
    y = torch.zeros((K, PH, PW, C), dtype=torch.float64)
    yabs = torch.zeros_like(y)
    terms = np.zeros(K, dtype=np.int64)
    for k in range(K):
        lv = int(levels[k])
        s = align_samples(rois[k], lv, PH, PW, sr, n_images, sizes, scales)
        if s is None:
            continue
        H, W = sizes[lv]
        gh, gw = s["g"]
        base = off[lv] + s["n"] * H * W
        acc = torch.zeros((PH * gh, PW * gw, C), dtype=torch.float64)
        aabs = torch.zeros_like(acc)
        for q in range(4):
            wq = torch.from_numpy(s["w"][q].astype(np.float64))[..., None]
            rows = torch.from_numpy(np.where(s["cell"][q] >= 0, base + s["cell"][q], 0))
            v = x[rows.reshape(-1)].view(PH * gh, PW * gw, C)
            acc += wq * v
            aabs += (wq * v).abs()
        cnt = float(gh * gw)
        y[k] = acc.view(PH, gh, PW, gw, C).sum(dim=(1, 3)) / cnt
        yabs[k] = aabs.view(PH, gh, PW, gw, C).sum(dim=(1, 3)) / cnt
        terms[k] = gh * gw
    return dict(y=y, yabs=yabs, terms=terms)


def roi_align_backward(dy, rois, levels, PH, PW, sr, n_images=N_IMAGES, sizes=SIZES, scales=SCALES):
    """dy [K, PH, PW, C] -> dict: dx [M, C] fp64 = sum of dy * w / count over the samples' corners (ROIAlign_cuda.cu:239-249),
    dxabs = the same sum of absolute values, terms [M] = number of (sample, corner) contributions per row"""
    dy = dy.double()
    K, C = len(rois), dy.shape[-1]
    off = row_offsets(n_images, sizes)
    M = off[-1]
    dx = torch.zeros((M, C), dtype=torch.float64)
    dxabs = torch.zeros_like(dx)
    terms = torch.zeros((M,), dtype=torch.int64)
    for k in range(K):
        lv = int(levels[k])
        s = align_samples(rois[k], lv, PH, PW, sr, n_images, sizes, scales)
        if s is None:
            continue
        H, W = sizes[lv]
        gh, gw = s["g"]
        base = off[lv] + s["n"] * H * W
        g = dy[k].view(PH, 1, PW, 1, C).expand(PH, gh, PW, gw, C).reshape(PH * gh * PW * gw, C)
        live = torch.from_numpy(s["live"].reshape(-1))
        for q in range(4):
            wq = torch.from_numpy(s["w"][q].astype(np.float64)).reshape(-1, 1)
            rows = torch.from_numpy(base + s["cell"][q]).reshape(-1)
            t = (g * wq / float(gh * gw))[live]
            dx.index_add_(0, rows[live], t)
            dxabs.index_add_(0, rows[live], t.abs())
            terms.index_add_(0, rows[live], torch.ones(int(live.sum()), dtype=torch.int64))
    return dict(dx=dx, dxabs=dxabs, terms=terms)


# ----------------------------------------------------------------------------- ROIPool
def _round_half_away(v):
    v = float(v)  # the fp32 product, exactly
    return int(np.sign(v) * np.floor(abs(v) + 0.5))


def pool_bins(roi, scale, PH, PW, H, W):
    """ROIPool_cuda.cu:30-56: per axis the clipped [start, end) of every bin"""
    r = np.asarray(roi, dtype=f32)
    s = f32(scale)
    sw, sh, ew, eh = (_round_half_away(r[i] * s) for i in (1, 2, 3, 4))
    rw, rh = max(ew - sw + 1, 1), max(eh - sh + 1, 1)
    bh, bw = f32(f32(rh) / f32(PH)), f32(f32(rw) / f32(PW))
    hb = [(min(max(int(np.floor(f32(p) * bh)) + sh, 0), H), min(max(int(np.ceil(f32(p + 1) * bh)) + sh, 0), H)) for p in range(PH)]
    wb = [(min(max(int(np.floor(f32(p) * bw)) + sw, 0), W), min(max(int(np.ceil(f32(p + 1) * bw)) + sw, 0), W)) for p in range(PW)]
    return hb, wb


def roi_pool(x, rois, levels, PH, PW, n_images=N_IMAGES, sizes=SIZES, scales=SCALES):
    """x [M, C] fp32 -> (y [K, PH, PW, C] fp32, argmax [K, PH, PW, C] int32): exact, no arithmetic on the values"""
    xn = x.float().numpy()
    K, C = len(rois), xn.shape[1]
    off = row_offsets(n_images, sizes)
    y = np.zeros((K, PH, PW, C), dtype=f32)
    am = np.full((K, PH, PW, C), -1, dtype=np.int32)
    for k in range(K):
        lv = int(levels[k])
        n = _place(rois[k], lv, n_images, len(sizes))
        if n is None:
            continue
        H, W = sizes[lv]
        img = xn[off[lv] + n * H * W: off[lv] + (n + 1) * H * W].reshape(H, W, C)
        hb, wb = pool_bins(rois[k], scales[lv], PH, PW, H, W)
        for ph, (hs, he) in enumerate(hb):
            for pw, (ws, we) in enumerate(wb):
                if he <= hs or we <= ws:
                    continue  # empty: 0 and -1
                win = img[hs:he, ws:we].reshape(-1, C)
                cells = (np.arange(hs, he)[:, None] * W + np.arange(ws, we)[None, :]).reshape(-1)
                first = np.argmax(win, axis=0)  # the first maximum in (h, w) scan order: a strict > keeps it
                best = win[first, np.arange(C)]
                ok = best > -FLT_MAX  # the start value is -FLT_MAX, compared with a strict >
                y[k, ph, pw] = np.where(ok, best, f32(-FLT_MAX))
                am[k, ph, pw] = np.where(ok, cells[first], -1)
    return torch.from_numpy(y), torch.from_numpy(am)


def roi_pool_backward(dy, argmax, rois, levels, n_images=N_IMAGES, sizes=SIZES):
    """dict: dx [M, C] fp64 (dy added at the argmax, ROIPool_cuda.cu:100-105), dxabs, terms [M, C] contributions per element"""
    dy = dy.double()
    K, PH, PW, C = dy.shape
    off = row_offsets(n_images, sizes)
    M = off[-1]
    dx = torch.zeros((M * C,), dtype=torch.float64)
    dxabs = torch.zeros_like(dx)
    terms = torch.zeros((M * C,), dtype=torch.int64)
    ch = torch.arange(C)
    for k in range(K):
        lv = int(levels[k])
        n = _place(rois[k], lv, n_images, len(sizes))
        if n is None:
            continue
        H, W = sizes[lv]
        a = argmax[k].long().reshape(-1, C)
        g = dy[k].reshape(-1, C)
        ok = a >= 0
        idx = ((off[lv] + n * H * W + a) * C + ch[None, :])[ok]
        dx.index_add_(0, idx, g[ok])
        dxabs.index_add_(0, idx, g[ok].abs())
        terms.index_add_(0, idx, torch.ones_like(idx))
    return dict(dx=dx.view(M, C), dxabs=dxabs.view(M, C), terms=terms.view(M, C))


# ----------------------------------------------------------------------------- error bounds, from the operation counts
# u = 2^-24 is the unit roundoff of fp32, gamma(n) = n u / (1 - n u) bounds the relative error of a quantity that passed
# through n roundings (Higham, Accuracy and Stability of Numerical Algorithms, Lemma 3.1).  The restatements use the SAME fp32
# weights as the code under test (they are inputs of the fp64 sums, exact there), so only the value arithmetic is bounded;
# the fp64 sums themselves err by about 2^-53 of the same absolute sums, which the "+ 1" below covers with room to spare.
# TINY covers products and quotients that underflow to subnormals (an absolute error of at most 2^-150 each).
U = 2.0 ** -24


def gamma(n):
    n = torch.as_tensor(n, dtype=torch.float64)
    return n * U / (1 - n * U)


def _tiny(n):
    return (torch.as_tensor(n, dtype=torch.float64) + 1) * 2.0 ** -149


def align_forward_bound(ref):
    """ROIAlign forward, per output element.  One sample is fl(fl(fl(p1 + p2) + p3) + p4) with p_q = fl(w_q v_q): a product
    passes through its own rounding and at most 3 sums, 4 roundings.  The n = g_h g_w samples are added to 0 one by one (the
    first addition is exact: n - 1 more roundings at most for any term), and one division follows: n + 4 roundings in all, so
    |y - y_exact| <= gamma(n + 4 + 1) * sum |w v| / count."""
    n = torch.from_numpy(ref["terms"]).double().view(-1, 1, 1, 1)
    return gamma(n + 5) * ref["yabs"] + _tiny(n + 5)


def align_backward_bound(ref):
    """ROIAlign data gradient, per element of dx.  A contribution is fl(fl(dy w) / count), 2 roundings; the m contributions
    of a row are added to 0 one by one (m - 1 roundings at most): m + 1 in all, |dx - dx_exact| <= gamma(m + 1 + 1) * sum
    |dy w / count|."""
    m = ref["terms"].double().view(-1, 1)
    return gamma(m + 2) * ref["dxabs"] + _tiny(m + 2)


def pool_backward_bound(ref):
    """ROIPool data gradient, per element: m values of dy added to 0 one by one, m - 1 roundings: gamma(m - 1 + 1) * sum |dy|"""
    m = ref["terms"].double()
    return gamma(m) * ref["dxabs"] + _tiny(m)


# ----------------------------------------------------------------------------- the ROI cases
def special_rois():
    """(roi, level, what) -- every case the tests must contain, on the pyramid above (image about 68 x 52)"""
    return [
        ((0, 9.0, 7.0, 41.0, 33.0), 0, "inside"),
        ((0, 500.0, 500.0, 600.0, 600.0), 0, "outside"),          # start beyond W and H: all zeros
        ((0, -400.0, -400.0, -300.0, -300.0), 0, "outside"),      # end below -1: all zeros
        ((0, -6.0, -6.0, 2.0, 2.0), 0, "border"),                 # (1, 1), sr 1: the sample sits at -0.5, inside (-1, 0]
        ((0, -8.0, -8.0, 0.0, 0.0), 0, "border"),                 # (1, 1), sr 1: exactly -1, still live
        ((0, 64.0, 48.0, 72.0, 56.0), 0, "border"),               # (1, 1), sr 1: y == H = 13 and x == W = 17 exactly
        ((0, -7.0, 20.0, 30.0, 61.0), 0, "border"),               # left and bottom
        ((0, 41.0, -9.0, 75.0, 18.0), 0, "border"),               # right and top
        ((0, 30.0, 30.0, 10.0, 10.0), 0, "x2 < x1"),              # forced to 1 x 1
        ((0, 10.3, 10.7, 10.9, 11.2), 0, "sub-pixel"),
        ((0, 0.0, 0.0, 68.0, 52.0), 0, "whole map"),              # adaptive grid 13 x 17 at (1, 1)
        ((1, -30.0, -30.0, 100.0, 90.0), 0, "beyond the map"),    # adaptive grid 30 x 33 at (1, 1), most samples outside
        ((1, 8.0, 8.0, 40.0, 36.0), 0, "second image"),
        ((-1, 8.0, 8.0, 40.0, 36.0), 0, "image -1"),
        ((2, 8.0, 8.0, 40.0, 36.0), 0, "image N"),
        ((0, 8.0, 8.0, 40.0, 36.0), 3, "level 3"),
        ((0, 8.0, 8.0, 40.0, 36.0), -1, "level -1"),
        ((0, 4.0, 4.0, 60.0, 50.0), 1, "level 1"),
        ((1, 0.0, 0.0, 72.0, 56.0), 2, "level 2"),
        ((1, -20.0, 10.0, 50.0, 90.0), 2, "level 2 border"),
        # ROIPool: bin edges exactly on integers (x1 * s = 2, x2 * s = 8: roi 7, (7, 7) bins of exactly 1), empty bins
        ((0, 8.0, 8.0, 32.0, 32.0), 0, "integer bins"),
        ((0, 60.0, 44.0, 90.0, 70.0), 0, "partly empty bins"),    # bins past the map's edge are empty
    ]


def make_rois(K, seed=0):
    """K ROIs: the special ones first, then 64 jittered around one box (they overlap on the same cells), then random ones on
    random levels and images.  Returns (rois fp32 [K, 5], levels int32 [K])."""
    rs = np.random.RandomState(seed)
    rois = [r for r, _, _ in special_rois()]
    lv = [l for _, l, _ in special_rois()]
    for _ in range(64):
        j = rs.uniform(-1.5, 1.5, 4)
        rois.append((1, 12.0 + j[0], 10.0 + j[1], 44.0 + j[2], 38.0 + j[3]))
        lv.append(0)
    while len(rois) < K:
        c = rs.uniform(-5, 75, 2)
        wh = np.exp(rs.uniform(np.log(2), np.log(70), 2))
        rois.append((int(rs.randint(0, 2)), c[0] - wh[0] / 2, c[1] - wh[1] / 2, c[0] + wh[0] / 2, c[1] + wh[1] / 2))
        lv.append(int(rs.randint(0, 3)))
    return torch.tensor(rois[:K], dtype=torch.float32).reshape(K, 5), torch.tensor(lv[:K], dtype=torch.int32)


def make_rows(C, seed=0, n_images=N_IMAGES, sizes=SIZES):
    M = row_offsets(n_images, sizes)[-1]
    return torch.randn(M, C, generator=torch.Generator().manual_seed(seed))
