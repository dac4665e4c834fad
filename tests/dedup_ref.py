"""The contract of csrc/dedup_hash.hip and framewright_amd/dedup.py: Pillow's 8-bit `convert('L')` and `resize(..., LANCZOS)` written
out in NumPy int64 and `math.sin`, the two frame hashes the reference's deduplicator builds on them, and its decision loop.

tests/test_dedup_ref_host.py holds this file byte for byte against Pillow itself; tests/test_dedup_gpu.py holds the device byte for
byte against this file.  Frames are uint8 H x W x 3 in BGR order, as everywhere in the project.

Pillow's resampler (8 bits per channel): a horizontal pass, then a vertical pass, each per channel, each writing uint8, a pass left
out when that size does not change.  The coefficients are float64: scale = in / out, fs = max(scale, 1), support = 3 fs; for output
index xx, center = (xx + 0.5) scale, the window is [xmin, xmax) = [max(int(center - support + 0.5), 0), min(int(center + support +
0.5), in)), w[x] = L((x + xmin - center + 0.5) / fs) with L(t) = sinc(t) sinc(t / 3) on -3 <= t < 3, the taps summed in tap order and
each divided by the sum.  The integer tap is int(w 2^22 +- 0.5) (away from zero), the output byte clamp((2^21 + sum px tap) >> 22).
"""
import hashlib
import math

import numpy as np

PRECISION_BITS = 22
KINDS = ("noise", "gradient", "blocks8", "constant")


def _sinc(t):
    if t == 0.0:
        return 1.0
    t = t * math.pi
    return math.sin(t) / t


def _lanczos(t):
    if -3.0 <= t < 3.0:
        return _sinc(t) * _sinc(t / 3)
    return 0.0


def ksize(in_size, out_size):
    """Taps a row of the table holds (Pillow's allocation; a window has at most this many)."""
    fs = max(in_size / out_size, 1.0)
    return int(math.ceil(3.0 * fs)) * 2 + 1


def taps(in_size, out_size):
    """(xmin[out], count[out], taps[out][ksize]) as int64; a row is zero behind its window."""
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = 3.0 * fs
    ks = ksize(in_size, out_size)
    xmin = np.zeros(out_size, np.int64)
    count = np.zeros(out_size, np.int64)
    table = np.zeros((out_size, ks), np.int64)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        lo = max(int(center - support + 0.5), 0)
        hi = min(int(center + support + 0.5), in_size)
        w = [_lanczos((x + lo - center + 0.5) / fs) for x in range(hi - lo)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        xmin[xx], count[xx] = lo, hi - lo
        for x, v in enumerate(w):
            table[xx, x] = int(v * (1 << PRECISION_BITS) + 0.5) if v >= 0 else int(v * (1 << PRECISION_BITS) - 0.5)
    return xmin, count, table


def _wrap32(s):
    """Pillow sums in int32: the wrapped value (no frame of uint8 pixels against normalised taps gets near the edge)."""
    return ((s + (1 << 31)) & 0xFFFFFFFF) - (1 << 31)


def _resize_axis(img, out_size, axis):
    """One pass along `axis` of a uint8 array; the pass is left out when the size stays."""
    in_size = img.shape[axis]
    if in_size == out_size:
        return img
    xmin, count, table = taps(in_size, out_size)
    src = np.moveaxis(img, axis, -1).astype(np.int64)
    out = np.empty(src.shape[:-1] + (out_size,), np.uint8)
    for xx in range(out_size):
        k = int(count[xx])
        s = (src[..., xmin[xx]:xmin[xx] + k] * table[xx, :k]).sum(axis=-1) + (1 << (PRECISION_BITS - 1))
        out[..., xx] = np.clip(_wrap32(s) >> PRECISION_BITS, 0, 255)
    return np.moveaxis(out, -1, axis)


def resize(img, out_w, out_h):
    """`Image.resize((out_w, out_h), LANCZOS)` of a uint8 H x W or H x W x C array: horizontal, then vertical."""
    return _resize_axis(_resize_axis(img, out_w, 1), out_h, 0)


def gray_bgr(img_bgr):
    """`convert('L')` of an RGB image held as BGR: (19595 R + 38470 G + 7471 B + 0x8000) >> 16."""
    p = img_bgr.astype(np.int64)
    return ((19595 * p[..., 2] + 38470 * p[..., 1] + 7471 * p[..., 0] + 0x8000) >> 16).astype(np.uint8)


def thumb(frame_bgr, out_w, out_h, gray_first):
    """uint8 out_h x out_w: gray then resize (the dHash thumbnail), or resize the three channels then gray (the pixel-hash one)."""
    if gray_first:
        return resize(gray_bgr(frame_bgr), out_w, out_h)
    return gray_bgr(resize(frame_bgr, out_w, out_h))


def dhash_bits(frame_bgr, hash_size=16):
    px = thumb(frame_bgr, hash_size + 1, hash_size, True)
    return (px[:, 1:] > px[:, :-1]).reshape(-1)


def bits_to_hex(bits):
    """The bits row-major, first bit most significant, as an integer in lower-case hex padded to ceil(len / 4) digits."""
    v = 0
    for b in bits:
        v = (v << 1) | int(b)
    return format(v, "0%dx" % ((len(bits) + 3) // 4))


def bits_to_bytes(bits):
    """The same integer, big-endian in ceil(len / 8) bytes: what fw_dhash_pack_u8 writes."""
    v = 0
    for b in bits:
        v = (v << 1) | int(b)
    return v.to_bytes((len(bits) + 7) // 8, "big")


def dhash_hex(frame_bgr, hash_size=16):
    return bits_to_hex(dhash_bits(frame_bgr, hash_size))


def hamming_hex(a, b):
    return bin(int(a, 16) ^ int(b, 16)).count("1")


def pixel_md5(frame_bgr, sample_rate=4):
    px = thumb(frame_bgr, 64, 64, False).reshape(-1)
    return hashlib.md5(bytes(px[::sample_rate].tolist())).hexdigest()


def similarity(h1, h2, perceptual, hash_size=16):
    if h1 == h2:
        return 1.0
    if perceptual:
        return 1.0 - hamming_hex(h1, h2) / (hash_size * hash_size)
    return 0.0


def analyze_hashes(hashes, perceptual, hash_size=16, threshold=0.98, target_fps=25.0):
    """The decision loop as plain data: frame 0 is unique; frame i repeats the LAST UNIQUE frame iff similarity >= threshold."""
    total = len(hashes)
    if total == 0:
        return dict(total_frames=0, unique_frames=0, duplicate_frames=0, detected_source_fps=0.0, target_fps=25.0,
                    frame_mapping={}, unique_indices=[])
    unique, mapping = [0], {0: 0}
    last_hash, last_idx = hashes[0], 0
    for i in range(1, total):
        if similarity(last_hash, hashes[i], perceptual, hash_size) >= threshold:
            mapping[i] = last_idx
        else:
            unique.append(i)
            mapping[i] = i
            last_hash, last_idx = hashes[i], i
    return dict(total_frames=total, unique_frames=len(unique), duplicate_frames=total - len(unique),
                detected_source_fps=target_fps * (len(unique) / total), target_fps=target_fps, frame_mapping=mapping,
                unique_indices=unique)


def analyze(frames, perceptual, hash_size=16, sample_rate=4, threshold=0.98, target_fps=25.0):
    hashes = [dhash_hex(f, hash_size) if perceptual else pixel_md5(f, sample_rate) for f in frames]
    return analyze_hashes(hashes, perceptual, hash_size, threshold, target_fps)


def make_frame(kind, h, w, seed=0):
    rng = np.random.default_rng(1000 * h + w + 7919 * seed)
    if kind == "noise":
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    if kind == "gradient":                                            # modular: wraps several times, a different period per channel
        y, x = np.mgrid[0:h, 0:w]
        return np.stack([(3 * x + 5 * y + 11 * seed) % 256, (7 * x + 2 * y + 40) % 256, (x * y + 13 * x) % 256], -1).astype(np.uint8)
    if kind == "blocks8":
        small = rng.integers(0, 256, ((h + 7) // 8, (w + 7) // 8, 3), dtype=np.uint8)
        return np.ascontiguousarray(np.repeat(np.repeat(small, 8, 0), 8, 1)[:h, :w])
    if kind == "constant":
        return np.full((h, w, 3), 200 - 3 * seed, np.uint8)
    raise ValueError(kind)


def make_clip(h, w):
    """Ten frames: distinct frames, an exact repeat, a repeat with +-1 on a sparse set of bytes, a run of three repeats."""
    a, b, c, d = make_frame("noise", h, w), make_frame("gradient", h, w), make_frame("blocks8", h, w), make_frame("noise", h, w, 1)
    near = b.astype(np.int16).reshape(-1)
    idx = np.arange(5, near.size, 97)
    near[idx] = np.clip(near[idx] + np.where(idx % 2 == 0, 1, -1), 0, 255)
    near = near.astype(np.uint8).reshape(b.shape)
    return np.stack([a, a.copy(), b, near, c, c.copy(), c.copy(), c.copy(), d, make_frame("constant", h, w)])
