"""References and shared inputs of the pointwise-kernel and cond-RNN tests (a helper module, not a conftest).

Every function states one kernel of scan_amd/csrc/pointwise.hip (plus scan_sgd_momentum_multi, scan_relu_backward and
scan_amd/csrc/condrnn.hip) the way its header comment does, as numpy slicing / loops or a torch-CPU loop; none calls the torch
op the kernel replaces -- tests/test_pointwise_host.py pins each of them against that op on the CPU.  Nothing here imports
scan_amd._lib.

Precision.  scale, add + ReLU, the ReLU backward, both pools, the FPN join, the take_images gradient and the column copy are
exact in fp32: the reference computes in fp32 and the GPU comparison is torch.equal.  downsample2x_sum adds in fp32 in the
kernel's documented association (g00 + g01) + (g10 + g11): also torch.equal.  SGD, the paradigm update and the cond RNN are
float64.

NHWC maps are numpy arrays [N, H, W, C]; ``rows(a)`` is the [N*H*W, C] matrix the kernels see.
"""
import numpy as np
import torch

F32 = np.float32


def rows(a):
    return np.ascontiguousarray(a).reshape(-1, a.shape[-1])


# ----------------------------------------------------------------------------- flat kernels
def scale(x, alpha):
    """y = alpha * x, one fp32 multiply per element"""
    return (F32(alpha) * np.asarray(x, F32)).astype(F32)


def add_relu(a, b):
    """y = max(a + b, 0): one fp32 add, one max"""
    s = np.asarray(a, F32) + np.asarray(b, F32)
    return np.where(s > 0, s, F32(0)).astype(F32)


def relu_backward(dy, y):
    """out = y > 0 ? dy : 0"""
    return np.where(np.asarray(y) > 0, np.asarray(dy, F32), F32(0)).astype(F32)


def sgd_step(p, g, buf, lr, wd, momentum, first):
    """one step of sgd_kernel in float64: gg = g + wd * w; b = first ? gg : momentum * buf + gg; buf <- b; p <- w - lr * b.
    On the first step buf is not read (it may hold anything).  Returns (p, buf)."""
    p, g = np.asarray(p, np.float64), np.asarray(g, np.float64)
    gg = g + float(wd) * p
    b = gg if first else float(momentum) * np.asarray(buf, np.float64) + gg
    return p - float(lr) * b, b


# ----------------------------------------------------------------------------- 2x2 / stride-2 max pooling
def _windows2(x):
    """the four window positions in window order: (0, 0), (0, 1), (1, 0), (1, 1)"""
    return x[:, 0::2, 0::2], x[:, 0::2, 1::2], x[:, 1::2, 0::2], x[:, 1::2, 1::2]


def maxpool2x2(x):
    a0, a1, a2, a3 = _windows2(np.asarray(x, F32))
    return np.maximum(np.maximum(a0, a1), np.maximum(a2, a3))


def maxpool2x2_backward(x, dy, relu_input=False):
    """dy goes to the FIRST position in window order that equals the window's maximum (-0.0 equals +0.0); relu_input: the
    result times (x > 0)."""
    x, dy = np.asarray(x, F32), np.asarray(dy, F32)
    m = maxpool2x2(x)
    dx = np.zeros_like(x)
    taken = np.zeros(m.shape, bool)
    for (oy, ox), a in zip(((0, 0), (0, 1), (1, 0), (1, 1)), _windows2(x)):
        hit = (a == m) & ~taken
        dx[:, oy::2, ox::2] = np.where(hit, dy, F32(0))
        taken |= hit
    assert taken.all()
    if relu_input:
        dx = np.where(x > 0, dx, F32(0))
    return dx


# windows built by hand, values at positions 0..3 -> the position that takes the gradient: ties (0,1), (1,2), (2,3), (1,3),
# (0,3), all four equal, -0.0 against +0.0 in both orders and off position 0, a tie of negatives, then a block of exact zeros
TIE_WINDOWS = (((5, 5, 1, 2), 0), ((1, 5, 5, 2), 1), ((1, 2, 5, 5), 2), ((1, 5, 2, 5), 1), ((5, 1, 2, 5), 0), ((3, 3, 3, 3), 0),
               ((-0.0, 0.0, -1, -2), 0), ((0.0, -0.0, -1, -2), 0), ((-1, -0.0, 0.0, -2), 1), ((-5, -1, -1, -3), 1)) \
    + (((0, 0, 0, 0), 0),) * 6


def tie_map(C):
    """x [1, 2, 2 * len(TIE_WINDOWS), C]: window i holds TIE_WINDOWS[i] times (1 + c % 3) in channel c (ties stay ties, zeros
    keep their sign)"""
    x = np.zeros((1, 2, 2 * len(TIE_WINDOWS), C), F32)
    s = (1 + np.arange(C) % 3).astype(F32)
    for i, (vals, _) in enumerate(TIE_WINDOWS):
        for p, v in enumerate(vals):
            x[0, p >> 1, 2 * i + (p & 1)] = F32(v) * s
    return x


# ----------------------------------------------------------------------------- 3x3 / stride 2 / pad 1 max pooling
def maxpool3x3s2(x):
    """out[n, yo, xo] = max over dy, dx in 0..2 of x[n, 2 yo - 1 + dy, 2 xo - 1 + dx], positions outside the map left out
    (they count as -inf, never as 0); Ho = (H - 1) / 2 + 1"""
    x = np.asarray(x, F32)
    N, H, W, C = x.shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    xp = np.full((N, 2 * Ho + 1, 2 * Wo + 1, C), -np.inf, F32)  # xp[yy + 1, xx + 1] = x[yy, xx]
    xp[:, 1:H + 1, 1:W + 1] = x
    out = np.full((N, Ho, Wo, C), -np.inf, F32)
    for dy in range(3):
        for dx in range(3):
            out = np.maximum(out, xp[:, dy:dy + 2 * Ho:2, dx:dx + 2 * Wo:2])
    return out


# ----------------------------------------------------------------------------- FPN top-down join
def upsample2x_add(lat, coarse):
    """y[n, yy, xx] = lat[n, yy, xx] + coarse[n, yy >> 1, xx >> 1]"""
    y = np.array(lat, F32)
    for oy in (0, 1):
        for ox in (0, 1):
            y[:, oy::2, ox::2] += np.asarray(coarse, F32)
    return y


def downsample2x_sum(g):
    """d[n, y, x] = (g[2y, 2x] + g[2y, 2x + 1]) + (g[2y + 1, 2x] + g[2y + 1, 2x + 1]), fp32, in this association"""
    g = np.asarray(g, F32)
    return (g[:, 0::2, 0::2] + g[:, 0::2, 1::2]) + (g[:, 1::2, 0::2] + g[:, 1::2, 1::2])


# ----------------------------------------------------------------------------- pyramids
def row_offsets(n_images, sizes):
    off = [0]
    for h, w in sizes:
        off.append(off[-1] + n_images * h * w)
    return off


def take_images(x, n_images, sizes, i0, i1):
    """rows of images [i0, i1) of every level, level-major"""
    ro = row_offsets(n_images, sizes)
    return np.concatenate([x[ro[l] + i0 * h * w:ro[l] + i1 * h * w] for l, (h, w) in enumerate(sizes)], 0)


def take_images_backward(g, n_images, sizes, i0, i1):
    """the full pyramid's gradient: the taken images' rows copied from g (the sub-pyramid's rows), every other row zero"""
    g = np.asarray(g, F32)
    ro = row_offsets(n_images, sizes)
    out = np.zeros((ro[-1], g.shape[1]), F32)
    o = 0
    for l, (h, w) in enumerate(sizes):
        for n in range(i0, i1):
            for r in range(h * w):
                out[ro[l] + n * h * w + r] = g[o]
                o += 1
    assert o == g.shape[0]
    return out


# ----------------------------------------------------------------------------- column block copy
def copy_cols(src, dst, ncols, ztail):
    """dst[r][c] = src[r][c] for c < ncols, zero for ncols <= c < ncols + ztail; every other column of dst is kept.  src / dst
    are 2-d arrays whose column 0 is the column the kernel's pointers are offset to."""
    out = np.array(dst, F32)
    out[:, :ncols] = np.asarray(src, F32)[:, :ncols]
    out[:, ncols:ncols + ztail] = 0
    return out


# ----------------------------------------------------------------------------- paradigm update
def paradigm_update(P, pb, it, dtype=np.float64):
    """P [K, C, T], pb [K, C], the counter value it in 0..T -> the new P (header of paradigm_update_kernel):
    slot = it - 1 if it == T else it; cur = P[:, :, slot]; m = sum_c (cur / max(|cur|, 1e-8)) (pb / max(|pb|, 1e-8));
    upd = cur * m + pb * (1 - m) where sum_c pb != 0, else cur; it == T: slots 0..T-2 <- slots 1..T-1; P[:, :, slot] = upd."""
    P, pb = np.array(P, dtype), np.asarray(pb, dtype)
    K, C, T = P.shape
    slot = it - 1 if it == T else it
    upd = np.empty((K, C), dtype)
    for k in range(K):
        cur, b = P[k, :, slot].copy(), pb[k]
        n_c = max(np.sqrt((cur * cur).sum()), dtype(1e-8))
        n_b = max(np.sqrt((b * b).sum()), dtype(1e-8))
        m = ((cur / n_c) * (b / n_b)).sum()
        upd[k] = cur * m + b * (1 - m) if b.sum() != 0 else cur
    if it == T:
        for t in range(T - 1):
            P[:, :, t] = P[:, :, t + 1]
    P[:, :, slot] = upd
    return P


PARADIGM_SHAPES = ((2, 256, 3), (32, 256, 3), (9, 1000, 3), (9, 1024, 2), (9, 5, 1))  # (K, C, T)
PARADIGM_EDGES = ("zero_current", "zero_batch", "plus_minus_one", "batch_is_current")


def paradigm_cases(K, C, T, it):
    """[(P, pb, {edge: class})]: fp32 inputs in which, in the slot this `it` updates, one class has an all-zero current row (a
    fresh prototype: the result is pb), one an all-zero batch row and one the batch row [1, -1, 0, ...] (non-zero entries that
    sum to exactly 0: both mean "class not seen"), and one a batch row equal to its current row (m = 1).  Each edge sits on a
    class of its own, so K = 2 takes two inputs for the four edges and a third of plain random rows; every other K one."""
    slot = it - 1 if it == T else it
    out = []
    for v, lo in enumerate(range(0, len(PARADIGM_EDGES), min(K, len(PARADIGM_EDGES)))):
        g = torch.Generator().manual_seed(1000 * K + 10 * C + 100003 * T + 7 * it + v)
        P = torch.randn(K, C, T, generator=g).numpy()
        pb = torch.randn(K, C, generator=g).numpy()
        where = {}
        for j, edge in enumerate(PARADIGM_EDGES[lo:lo + K]):
            k = (K - 1 - 2 * j) % K if K >= 4 else j  # spread over the classes, the last one (the last workgroup) included
            where[edge] = k
            if edge == "zero_current":
                P[k, :, slot] = 0
            elif edge == "zero_batch":
                pb[k] = 0
            elif edge == "plus_minus_one":
                pb[k] = 0
                pb[k, 0], pb[k, 1] = 1, -1
            else:
                pb[k] = P[k, :, slot]
        assert len(set(where.values())) == len(where)
        out.append((P, pb, where))
    if K < len(PARADIGM_EDGES):  # the edges took every class: one more input of plain random rows
        g = torch.Generator().manual_seed(1000 * K + 10 * C + 100003 * T + 7 * it + len(out))
        out.append((torch.randn(K, C, T, generator=g).numpy(), torch.randn(K, C, generator=g).numpy(), {}))
    return out


def paradigm_update_torch(P, pb, it):
    """the torch spelling of modeling/condgraph.py update_prototype_nx1_rnn (F.cosine_similarity, torch.where) in the dtype of
    its inputs"""
    import torch.nn.functional as F
    P = P.clone()
    T = P.shape[2]
    exist = pb.sum(-1).bool()[:, None]
    slot = it - 1 if it == T else it
    cur = P[:, :, slot]
    m = F.cosine_similarity(cur, pb).unsqueeze(1)
    upd = torch.where(exist, cur * m + pb * (1 - m), cur)
    if it == T:
        for i in range(it - 1):
            P[:, :, i] = P[:, :, i + 1]
    P[:, :, slot] = upd
    return P


# ----------------------------------------------------------------------------- cond RNN
COND_RNN_NAMES = ("wih0", "whh0", "bih0", "bhh0", "wih1", "whh1", "bih1", "bhh1", "wc", "bc")
COND_RNN_CASES = ((1, 1, 0.05), (1, 3, 0.05), (2, 2, 0.05), (9, 2, 0.05), (9, 3, 0.05), (9, 3, 0.1))  # (K, T, weight scale)


def cond_rnn_inputs(K, T, scale):
    """x [T, K, 256] (the paradigm, slot-major), the ten fp32 parameters in scan_cond_rnn_forward's order, dkernels [K, 256]"""
    g = torch.Generator().manual_seed(100 * K + T + int(round(1000 * scale)))
    x = torch.randn(T, K, 256, generator=g)
    shapes = ((512, 256), (512, 512), (512,), (512,), (512, 512), (512, 512), (512,), (512,), (256, 512, T), (256,))
    weights = [torch.randn(*s, generator=g) * scale for s in shapes]
    dk = torch.randn(K, 256, generator=g)
    return x, weights, dk


def cond_rnn(x, weights, dk, dtype=torch.float64):
    """the loop of condrnn.hip's header in ``dtype``:
        h0_t = tanh(x_t wih0^T + bih0 + bhh0 + h0_{t-1} whh0^T),  h1_t = tanh(h0_t wih1^T + bih1 + bhh1 + h1_{t-1} whh1^T),
        kernels[k][o] = bc[o] + sum_{c, t} wc[o][c][t] h1_t[k][c]
    with h_{-1} = 0.  Returns (kernels [K, 256], h0 [T, K, 512], h1 [T, K, 512], the ten gradients of sum(kernels * dk))."""
    x, dk = x.to(dtype), dk.to(dtype)
    w = [t.detach().to(dtype).requires_grad_(True) for t in weights]
    wih0, whh0, bih0, bhh0, wih1, whh1, bih1, bhh1, wc, bc = w
    T, K = x.shape[0], x.shape[1]
    h0, h1 = [], []
    for layer, (wih, whh, bih, bhh, hs) in enumerate(((wih0, whh0, bih0, bhh0, h0), (wih1, whh1, bih1, bhh1, h1))):
        for t in range(T):
            inp = x[t] if layer == 0 else h0[t]
            pre = inp @ wih.t() + bih + bhh
            if t > 0:
                pre = pre + hs[t - 1] @ whh.t()
            hs.append(torch.tanh(pre))
    ker = bc.expand(K, 256)
    for t in range(T):
        ker = ker + h1[t] @ wc[:, :, t].t()
    grads = torch.autograd.grad((ker * dk).sum(), w, allow_unused=True)
    grads = [torch.zeros_like(p) if gr is None else gr for p, gr in zip(w, grads)]  # T = 1: nothing reaches whh
    return ker.detach(), torch.stack(h0).detach(), torch.stack(h1).detach(), grads
