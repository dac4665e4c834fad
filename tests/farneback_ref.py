"""TEST INFRASTRUCTURE ONLY (imported by tests/ and nothing on the product path).

numpy restatement of the dense optical flow the reference's classical temporal denoise consumes,
src/framewright/processors/temporal_denoise.py:294-305: cv2.calcOpticalFlowFarneback(gray1, gray2, None, pyr_scale 0.5,
levels 3, winsize 15, iterations 3, poly_n 5, poly_sigma 1.1, flags 0), and of `_compute_flow_confidence` (:406-438).
OpenCV is not installed where this is built, so the algorithm is restated from OpenCV 4.x's published source
(modules/video/src/optflowgf.cpp: FarnebackOpticalFlowImpl::calc, FarnebackPrepareGaussian, FarnebackPolyExp,
FarnebackUpdateMatrices, FarnebackUpdateFlow_Blur; imgproc's GaussianBlur and resize for the pyramid) and bit-parity with cv2
is UNPINNED.  What it is for: `dtype=np.float64` is the contract the device kernels (csrc/optical_flow.hip) are held to,
`dtype=np.float32` is the same sequence of operations with every intermediate rounded to single precision - the yardstick for
what fp32 arithmetic costs on a given input.

Conventions shared by both dtypes and by the device code: the filter coefficients (Gaussian taps, g / x g / x^2 g, the border
ramp, the bilinear fractions) are the float32 values OpenCV holds them in; only the arithmetic on the image data changes with
`dtype`.  Details where OpenCV differs from the short description usually given of the algorithm, followed here:
  * FarnebackUpdateMatrices, sample point outside the second image: the second image contributes NOTHING to b (r2 = r3 = 0, so
    b = R0.b / 2), A is the first image's own, A_xy is halved - not "the first image's values for everything";
  * FarnebackPolyExp sums its horizontal pass, and FarnebackUpdateFlow_Blur its running box sums, in double; here both are sums
    in `dtype` (the device is all fp32), and the box mean is 15 direct taps, never a frame-long running sum;
  * the pyramid images are blurred at FULL resolution (GaussianBlur(ksize, sigma) with ksize = max(cvRound(5 sigma) | 1, 3),
    cvRound = round half to even: 3, 3, 9, 19 taps for scales 1, 1/2, 1/4, 1/8) and then resized INTER_LINEAR to the level size;
  * GaussianBlur with sigma = 0 (the finest level) takes the fixed 3-tap kernel [1/4, 1/2, 1/4];
  * resize computes the source coordinate in double, rounds it to float, and clamps: (float)((dx + 0.5) * scale - 0.5).
"""
import numpy as np

BORDER = np.array([0.14, 0.14, 0.4472, 0.4472, 0.4472], np.float32)     # FarnebackUpdateMatrices


def cv_round(x: float) -> int:
    """cvRound: round half to even."""
    return int(np.rint(x))


def bgr2gray_u8(img: np.ndarray) -> np.ndarray:
    """cv2.cvtColor(BGR2GRAY) on uint8 (temporal_denoise.py:290-291): 14-bit weights."""
    b, g, r = (img[:, :, i].astype(np.int64) for i in range(3))
    return ((b * 1868 + g * 9617 + r * 4899 + (1 << 13)) >> 14).astype(np.uint8)


def usable_levels(h: int, w: int, levels: int = 3, pyr_scale: float = 0.5) -> int:
    """FarnebackOpticalFlowImpl::calc, "Crop unnecessary levels": the pyramid runs k = usable .. 0."""
    scale, k = 1.0, 0
    while k < levels:
        scale *= pyr_scale
        if w * scale < 32 or h * scale < 32:
            break
        k += 1
    return k


def level_plan(h: int, w: int, levels: int = 3, pyr_scale: float = 0.5):
    """[(k, scale, sigma, ksize, level_h, level_w)] from the coarsest level to k = 0."""
    out = []
    for k in range(usable_levels(h, w, levels, pyr_scale), -1, -1):
        scale = 1.0
        for _ in range(k):
            scale *= pyr_scale
        sigma = (1.0 / scale - 1.0) * 0.5
        ksize = max(cv_round(sigma * 5) | 1, 3)
        out.append((k, scale, sigma, ksize, cv_round(h * scale), cv_round(w * scale)))
    return out


def gaussian_taps(ksize: int, sigma: float) -> np.ndarray:
    """cv::getGaussianKernel(ksize, sigma, CV_32F): the fixed table for sigma <= 0 and small odd ksize, else exp(-x^2 / 2 sigma^2)
    normalised in double and stored as float."""
    fixed = {1: [1.0], 3: [0.25, 0.5, 0.25], 5: [0.0625, 0.25, 0.375, 0.25, 0.0625],
             7: [0.03125, 0.109375, 0.21875, 0.28125, 0.21875, 0.109375, 0.03125]}
    if sigma <= 0 and ksize in fixed:
        return np.array(fixed[ksize], np.float32)
    if sigma <= 0:
        sigma = ((ksize - 1) * 0.5 - 1) * 0.3 + 0.8
    x = np.arange(ksize, dtype=np.float64) - (ksize - 1) * 0.5
    k = np.exp(-0.5 / (sigma * sigma) * x * x)
    total = 0.0
    for v in k:                                                # summed in tap order, as OpenCV does
        total += float(v)
    return (k / total).astype(np.float32)


def gaussian_blur(img: np.ndarray, ksize: int, sigma: float, dtype) -> np.ndarray:
    """cv2.GaussianBlur on a float image, BORDER_REFLECT_101: rows, then columns, symmetric form k0 c + sum k_i (r_i + l_i)."""
    k = gaussian_taps(ksize, sigma).astype(dtype)
    r = ksize // 2

    def rows(a):
        w = a.shape[1]
        p = np.pad(a, ((0, 0), (r, r)), mode="reflect")
        acc = k[r] * p[:, r:r + w]
        for i in range(1, r + 1):
            acc = acc + k[r + i] * (p[:, r + i:r + i + w] + p[:, r - i:r - i + w])
        return acc

    return rows(rows(img.astype(dtype)).T).T


def _resize_axis(dn: int, sn: int):
    scale = 1.0 / (float(dn) / float(sn))                      # inv_scale = dsize / ssize; scale = 1 / inv_scale (double)
    f = ((np.arange(dn, dtype=np.float64) + 0.5) * scale - 0.5).astype(np.float32)
    s = np.floor(f).astype(np.int64)
    f = f - s.astype(np.float32)
    lo, hi = s < 0, s >= sn - 1
    f = np.where(lo | hi, np.float32(0), f).astype(np.float32)
    s = np.where(lo, 0, np.where(hi, sn - 1, s))
    return s, np.minimum(s + 1, sn - 1), f


def resize_linear(src: np.ndarray, dh: int, dw: int, dtype) -> np.ndarray:
    """cv2.resize(INTER_LINEAR) on a float image: horizontal pass S[sx] (1 - fx) + S[sx + 1] fx, then the vertical one."""
    sh, sw = src.shape
    x0, x1, fx = _resize_axis(dw, sw)
    y0, y1, fy = _resize_axis(dh, sh)
    fx, fy = fx.astype(dtype), fy.astype(dtype)
    one = dtype(1)
    src = src.astype(dtype)
    hz = src[:, x0] * (one - fx)[None, :] + src[:, x1] * fx[None, :]
    return hz[y0, :] * (one - fy)[:, None] + hz[y1, :] * fy[:, None]


def prepare_gaussian(n: int = 5, sigma: float = 1.1):
    """FarnebackPrepareGaussian: g, x g, x^2 g (float, index k = 0 .. n is offset k) and the four entries of the inverse Gram matrix
    of {1, x, y, x^2, y^2, xy} under g(x) g(y) (double)."""
    if sigma < np.finfo(np.float32).eps:
        sigma = n * 0.3
    xs = np.arange(-n, n + 1)
    g = np.exp(-(xs * xs) / (2 * sigma * sigma)).astype(np.float32)
    s = 0.0
    for v in g:
        s += float(v)
    s = 1.0 / s
    g = (g.astype(np.float64) * s).astype(np.float32)
    xg = (xs.astype(np.float32) * g).astype(np.float32)
    xxg = ((xs * xs).astype(np.float32) * g).astype(np.float32)
    G = np.zeros((6, 6), np.float64)
    f32 = np.float32
    for yi, y in enumerate(xs):
        for xi, x in enumerate(xs):
            gg = f32(g[yi] * g[xi])                            # float products, double accumulation, as in OpenCV
            G[0, 0] += gg
            G[1, 1] += f32(f32(gg * f32(x)) * f32(x))
            G[3, 3] += f32(f32(f32(f32(gg * f32(x)) * f32(x)) * f32(x)) * f32(x))
            G[5, 5] += f32(f32(f32(f32(gg * f32(x)) * f32(x)) * f32(y)) * f32(y))
    G[2, 2] = G[0, 3] = G[0, 4] = G[3, 0] = G[4, 0] = G[1, 1]
    G[4, 4] = G[3, 3]
    G[3, 4] = G[4, 3] = G[5, 5]
    inv = np.linalg.inv(G)
    return g[n:], xg[n:], xxg[n:], (inv[1, 1], inv[0, 3], inv[3, 3], inv[5, 5])


def poly_exp(src: np.ndarray, dtype, n: int = 5, sigma: float = 1.1) -> np.ndarray:
    """FarnebackPolyExp -> [5][H][W] planes (b_y, b_x, A_yy, A_xx, A_xy); replicate border."""
    g, xg, xxg, ig = prepare_gaussian(n, sigma)
    g, xg, xxg = g.astype(dtype), xg.astype(dtype), xxg.astype(dtype)
    ig11, ig03, ig33, ig55 = (dtype(np.float32(v)) if dtype == np.float32 else dtype(v) for v in ig)
    h, w = src.shape
    p = np.pad(src.astype(dtype), ((n, n), (0, 0)), mode="edge")
    r0 = p[n:n + h] * g[0]
    r1 = np.zeros_like(r0)
    r2 = np.zeros_like(r0)
    for k in range(1, n + 1):
        s0, s1 = p[n - k:n - k + h], p[n + k:n + k + h]
        t = s0 + s1
        r0 = r0 + g[k] * t
        r1 = r1 + xg[k] * (s1 - s0)
        r2 = r2 + xxg[k] * t
    q0, q1, q2 = (np.pad(r, ((0, 0), (n, n)), mode="edge") for r in (r0, r1, r2))
    c = slice(n, n + w)
    b1, b3, b5 = q0[:, c] * g[0], q1[:, c] * g[0], q2[:, c] * g[0]
    b2 = np.zeros_like(b1)
    b4 = np.zeros_like(b1)
    b6 = np.zeros_like(b1)
    for k in range(1, n + 1):
        pl, mi = slice(n + k, n + k + w), slice(n - k, n - k + w)
        tg = q0[:, pl] + q0[:, mi]
        b1 = b1 + tg * g[k]
        b4 = b4 + tg * xxg[k]
        b2 = b2 + (q0[:, pl] - q0[:, mi]) * xg[k]
        b3 = b3 + (q1[:, pl] + q1[:, mi]) * g[k]
        b6 = b6 + (q1[:, pl] - q1[:, mi]) * xg[k]
        b5 = b5 + (q2[:, pl] + q2[:, mi]) * g[k]
    return np.stack([b3 * ig11, b2 * ig11, b1 * ig03 + b5 * ig33, b1 * ig03 + b4 * ig33, b6 * ig55]).astype(dtype)


def update_matrices(R0: np.ndarray, R1: np.ndarray, fx: np.ndarray, fy: np.ndarray, dtype) -> np.ndarray:
    """FarnebackUpdateMatrices -> [5][H][W] planes (G11, G12, G22, h1, h2)."""
    _, h, w = R0.shape
    xs, ys = np.meshgrid(np.arange(w), np.arange(h))
    dx, dy = fx.astype(dtype), fy.astype(dtype)
    px, py = xs.astype(dtype) + dx, ys.astype(dtype) + dy
    with np.errstate(invalid="ignore"):
        x1f, y1f = np.floor(px), np.floor(py)
        inside = (x1f >= 0) & (x1f < w - 1) & (y1f >= 0) & (y1f < h - 1)
    x1 = np.where(inside, x1f, 0).astype(np.int64)
    y1 = np.where(inside, y1f, 0).astype(np.int64)
    ax, ay = np.where(inside, px - x1f, 0).astype(dtype), np.where(inside, py - y1f, 0).astype(dtype)
    one, half, quarter = dtype(1), dtype(0.5), dtype(0.25)
    a00, a01, a10, a11 = (one - ax) * (one - ay), ax * (one - ay), (one - ax) * ay, ax * ay
    x2, y2 = np.minimum(x1 + 1, w - 1), np.minimum(y1 + 1, h - 1)
    s = [a00 * R1[c][y1, x1] + a01 * R1[c][y1, x2] + a10 * R1[c][y2, x1] + a11 * R1[c][y2, x2] for c in range(5)]
    r2 = np.where(inside, s[0], 0)
    r3 = np.where(inside, s[1], 0)
    r4 = np.where(inside, (R0[2] + s[2]) * half, R0[2])
    r5 = np.where(inside, (R0[3] + s[3]) * half, R0[3])
    r6 = np.where(inside, (R0[4] + s[4]) * quarter, R0[4] * half)
    r2 = (R0[0] - r2) * half
    r3 = (R0[1] - r3) * half
    r2 = r2 + (r4 * dy + r6 * dx)
    r3 = r3 + (r6 * dy + r5 * dx)

    def ramp(n):
        i = np.arange(n)
        lo = np.where(i < 5, BORDER[np.minimum(i, 4)], np.float32(1))
        hi = np.where(i >= n - 5, BORDER[np.clip(n - i - 1, 0, 4)], np.float32(1))
        return lo.astype(np.float32), hi.astype(np.float32)

    xl, xh = ramp(w)
    yl, yh = ramp(h)
    scale = (((xl * xh)[None, :] * yl[:, None]).astype(np.float32) * yh[:, None]).astype(np.float32).astype(dtype)
    r2, r3, r4, r5, r6 = (v.astype(dtype) * scale for v in (r2, r3, r4, r5, r6))
    return np.stack([r4 * r4 + r6 * r6, (r4 + r5) * r6, r5 * r5 + r6 * r6, r4 * r2 + r6 * r3, r6 * r2 + r5 * r3]).astype(dtype)


def box_mean(a: np.ndarray, winsize: int, dtype) -> np.ndarray:
    """winsize x winsize mean, replicate border: winsize direct taps down the columns, then along the rows, then the scale."""
    m = winsize // 2
    h, w = a.shape
    p = np.pad(a.astype(dtype), ((m, m), (m, m)), mode="edge")
    v = p[0:h]
    for j in range(1, winsize):
        v = v + p[j:j + h]
    o = v[:, 0:w]
    for j in range(1, winsize):
        o = o + v[:, j:j + w]
    return o * dtype(np.float32(1.0 / (winsize * winsize)))


def solve_flow(M: np.ndarray, winsize: int, dtype):
    """The flow half of FarnebackUpdateFlow_Blur: box mean of the five planes, then the 2 x 2 solve with the 1e-3 ridge."""
    g11, g12, g22, h1, h2 = (box_mean(M[c], winsize, dtype) for c in range(5))
    idet = dtype(1) / (g11 * g22 - g12 * g12 + dtype(np.float32(1e-3)))
    return ((g11 * h2 - g12 * h1) * idet).astype(dtype), ((g22 * h1 - g12 * h2) * idet).astype(dtype)


def farneback(img1: np.ndarray, img2: np.ndarray, dtype=np.float64, pyr_scale: float = 0.5, levels: int = 3, winsize: int = 15,
              iterations: int = 3, poly_n: int = 5, poly_sigma: float = 1.1):
    """cv2.calcOpticalFlowFarneback(gray1, gray2, None, pyr_scale, levels, winsize, iterations, poly_n, poly_sigma, 0) for uint8
    gray (H x W) or BGR (H x W x 3) frames -> (flow_x, flow_y) in `dtype`."""
    dtype = np.dtype(dtype).type
    gray = [bgr2gray_u8(i) if i.ndim == 3 else i for i in (img1, img2)]
    h, w = gray[0].shape
    fx = fy = None
    for k, scale, sigma, ksize, lh, lw in level_plan(h, w, levels, pyr_scale):
        if fx is None:
            fx, fy = np.zeros((lh, lw), dtype), np.zeros((lh, lw), dtype)
        else:
            mul = dtype(1.0 / pyr_scale)
            fx, fy = resize_linear(fx, lh, lw, dtype) * mul, resize_linear(fy, lh, lw, dtype) * mul
        R = [poly_exp(resize_linear(gaussian_blur(g.astype(dtype), ksize, sigma, dtype), lh, lw, dtype), dtype, poly_n, poly_sigma)
             for g in gray]
        M = update_matrices(R[0], R[1], fx, fy, dtype)
        for i in range(iterations):
            fx, fy = solve_flow(M, winsize, dtype)
            if i < iterations - 1:
                M = update_matrices(R[0], R[1], fx, fy, dtype)
    return fx, fy


def flow_variance(fx: np.ndarray, fy: np.ndarray, dtype=np.float64) -> np.ndarray:
    """temporal_denoise.py:420-431: cv2.filter2D(., -1, ones((5, 5)) / 25) (BORDER_REFLECT_101; the kernel is held as float32, the 25
    products summed row by row) of each component, of the squared deviations, var_x + var_y."""
    dtype = np.dtype(dtype).type
    kf = dtype(np.float32(1.0 / 25.0))

    def box(a):
        h, w = a.shape
        p = np.pad(a, 2, mode="reflect")
        acc = np.zeros((h, w), dtype)
        for dy in range(5):
            for dx in range(5):
                acc = acc + kf * p[dy:dy + h, dx:dx + w]
        return acc

    fx, fy = fx.astype(dtype), fy.astype(dtype)
    ex, ey = fx - box(fx), fy - box(fy)
    return box(ex * ex) + box(ey * ey)


def flow_confidence(flow, dtype=np.float64) -> np.ndarray:
    """`_compute_flow_confidence` (temporal_denoise.py:406-438); flow: H x W x 2 or (flow_x, flow_y)."""
    dtype = np.dtype(dtype).type
    fx, fy = (flow[..., 0], flow[..., 1]) if isinstance(flow, np.ndarray) else flow
    var = flow_variance(fx, fy, dtype)
    max_var = dtype(np.percentile(var, 95)) + dtype(1e-6)
    return (dtype(1) - np.clip(var / max_var, 0, 1)).astype(dtype)


def flow_magnitude_f32(fx: np.ndarray, fy: np.ndarray) -> np.ndarray:
    """temporal_denoise.py:320 on the float32 maps cv2 returns: every operation rounded on its own."""
    fx, fy = fx.astype(np.float32), fy.astype(np.float32)
    return np.sqrt(fx ** 2 + fy ** 2)


# ---- inputs shared by the host and the GPU tests ------------------------------------------------------------------------------
def texture_fn(seed: int, size: int = 1024, sigma: float = 3.0):
    """A band-limited random texture that can be sampled anywhere: seeded noise, Gaussian-smoothed (periodic), scaled to 0 - 255,
    returned as a function (ys, xs) -> values by periodic bilinear lookup of the smooth field."""
    rng = np.random.default_rng(seed)
    f = np.fft.rfft2(rng.standard_normal((size, size)))
    ky, kx = np.fft.fftfreq(size)[:, None], np.fft.rfftfreq(size)[None, :]
    t = np.fft.irfft2(f * np.exp(-2 * (np.pi * sigma) ** 2 * (kx * kx + ky * ky)), s=(size, size))
    t = (t - t.min()) / (t.max() - t.min()) * 255.0

    def sample(ys, xs):
        y0, x0 = np.floor(ys).astype(np.int64), np.floor(xs).astype(np.int64)
        ay, ax = ys - y0, xs - x0
        y0, x0, y1, x1 = y0 % size, x0 % size, (y0 + 1) % size, (x0 + 1) % size
        return (t[y0, x0] * (1 - ax) + t[y0, x1] * ax) * (1 - ay) + (t[y1, x0] * (1 - ax) + t[y1, x1] * ax) * ay

    return sample


def moving_pair(h: int, w: int, motion, seed: int = 11):
    """Two uint8 gray frames of one texture: frame2(p) = frame1(p - d(p)), so the true flow from frame1 to frame2 is d.
    motion = ("shift", dx, dy) or ("affine", angle_rad, zoom) about the image centre -> (frame1, frame2, true_fx, true_fy)."""
    tex = texture_fn(seed)
    ys, xs = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    if motion[0] == "shift":
        dx, dy = np.full((h, w), float(motion[1])), np.full((h, w), float(motion[2]))
        sx, sy = xs - dx, ys - dy
    else:
        _, ang, zoom = motion
        cy, cx = (h - 1) / 2.0, (w - 1) / 2.0
        c, s = np.cos(ang) * zoom, np.sin(ang) * zoom
        # forward map p -> q = C + A (p - C); frame2(q) = frame1(p): sample frame1 at the inverse map of the grid
        det = c * c + s * s
        ux, uy = xs - cx, ys - cy
        sx, sy = cx + (c * ux + s * uy) / det, cy + (-s * ux + c * uy) / det
        # true flow at p (frame1 coordinates): q - p
        dx, dy = (c * ux - s * uy) - ux, (s * ux + c * uy) - uy
    off = 300.0                                                # keep the periodic lookup away from the wrap for any motion
    f1 = np.clip(np.rint(tex(ys + off, xs + off)), 0, 255).astype(np.uint8)
    f2 = np.clip(np.rint(tex(sy + off, sx + off)), 0, 255).astype(np.uint8)
    return f1, f2, dx, dy


def gpu_cases():
    """The inputs of the device-against-contract test (tests/test_flow_gpu.py) and of the single-precision-cost test
    (tests/test_flow_ref_host.py): (name, frame1, frame2); gray H x W or BGR H x W x 3 uint8."""
    from framewright_amd.synth import synthetic_frames
    cases = []
    for (h, w), motion in [((45, 67), ("shift", 0.6, -0.4)), ((96, 128), ("shift", 1.5, 1.0)), ((271, 483), ("shift", -3.25, 2.5)),
                           ((271, 483), ("affine", 0.01, 1.01)), ((540, 960), ("shift", 4.5, -3.0)),
                           ((1080, 1920), ("shift", -2.5, 1.5))]:
        f1, f2, _, _ = moving_pair(h, w, motion)
        cases.append((f"texture_{h}x{w}_{motion[0]}", f1, f2))
    f1, f2, _, _ = moving_pair(96, 128, ("shift", -1.0, 0.75), seed=5)
    cases.append(("texture_bgr_96x128", np.stack([f1, np.roll(f1, 3, 1), f1[::-1]], 2).copy(),
                  np.stack([f2, np.roll(f2, 3, 1), f2[::-1]], 2).copy()))
    for (h, w) in [(96, 128), (271, 483)]:
        a, b = synthetic_frames(2, h, w, seed=h)[:2]
        cases.append((f"synthetic_bgr_{h}x{w}", np.ascontiguousarray(a), np.ascontiguousarray(b)))
    return cases
