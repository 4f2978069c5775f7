"""The float64 reference and the case table of the image-metric tests (test_image_metrics_cpu.py,
test_image_metrics_gpu.py).

The SSIM reference is the DIRECT form of the definition (include/hashmod.h, DESIGN.md "Image metrics on the device"):
for every window position the explicit win x win weighted sums of x, y, x^2, y^2, x y - no separable passes and no
library filter - so it shares nothing with how the kernel is organised.  Inputs are seeded numpy arrays."""
import functools
import zlib

import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

K1, K2 = 0.01, 0.03


def window(win=11, sigma=1.5):
    """[win, win] fp64 weights g(i) g(j), g(r) ~ exp(-(r - (win-1)/2)^2 / (2 sigma^2)) normalised to sum 1"""
    r = np.arange(win, dtype=np.float64) - (win - 1) / 2.0
    g = np.exp(-(r * r) / (2.0 * sigma * sigma))
    g /= g.sum()
    return np.outer(g, g)


def ssim_ref(x, y, L=1.0, win=11, sigma=1.5):
    """(ssim [B], map [B, H-win+1, W-win+1, C]) in float64 of x, y [B, H, W, C]"""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    assert x.shape == y.shape and x.ndim == 4 and min(x.shape[1:3]) >= win
    w2 = window(win, sigma)
    c1, c2 = (K1 * L) ** 2, (K2 * L) ** 2

    def moment(img):                                    # [B, H, W, C] -> [B, OH, OW, C]
        v = sliding_window_view(img, (win, win), axis=(1, 2))      # [B, OH, OW, C, win, win]
        return (v * w2).sum(axis=(-2, -1))

    mx, my = moment(x), moment(y)
    sx2 = moment(x * x) - mx * mx
    sy2 = moment(y * y) - my * my
    sxy = moment(x * y) - mx * my
    s = ((2.0 * mx * my + c1) * (2.0 * sxy + c2)) / ((mx * mx + my * my + c1) * (sx2 + sy2 + c2))
    return s.mean(axis=(1, 2, 3)), s


def ssim_scipy(x, y, L=1.0, win=11, sigma=1.5):
    """the same map through scipy's separable filter (gaussian_filter, reflect, truncate 3.5: an 11-tap window for
    sigma 1.5), border cropped - the formulation of skimage / torchmetrics; only to cross-check ssim_ref"""
    from scipy.ndimage import gaussian_filter
    assert win == 2 * int(3.5 * sigma + 0.5) + 1
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    c1, c2 = (K1 * L) ** 2, (K2 * L) ** 2
    pad = (win - 1) // 2

    def moment(img):
        f = gaussian_filter(img, sigma=(0, sigma, sigma, 0), truncate=3.5, mode="reflect")
        return f[:, pad:img.shape[1] - pad, pad:img.shape[2] - pad, :]

    mx, my = moment(x), moment(y)
    sx2 = moment(x * x) - mx * mx
    sy2 = moment(y * y) - my * my
    sxy = moment(x * y) - mx * my
    return ((2.0 * mx * my + c1) * (2.0 * sxy + c2)) / ((mx * mx + my * my + c1) * (sx2 + sy2 + c2))


def psnr_ref(x, y, mask=None, L=1.0):
    """(psnr [B], mse [B], n [B]) in float64: mse = sum over set pixels and channels of (x - y)^2 / (n C);
    mse == 0 -> +inf, n == 0 -> nan"""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    B, H, W, C = x.shape
    m = np.ones((B, H, W), bool) if mask is None else np.asarray(mask) != 0
    d2 = np.where(m[..., None], (x - y) ** 2, 0.0)
    n = m.reshape(B, -1).sum(1).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        mse = d2.reshape(B, -1).sum(1) / (n * C)
        psnr = 10.0 * np.log10(L * L / mse)
    return psnr, mse, n


# ---------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------
CONTENTS = ("noise", "blur", "dark")


def _smooth(a):
    """5 x 5 box blur with edge replication along H and W of [B, H, W, C]"""
    for axis in (1, 2):
        p = np.pad(a, [(2, 2) if ax == axis else (0, 0) for ax in range(4)], mode="edge")
        a = sum(np.take(p, np.arange(k, k + a.shape[axis]), axis=axis) for k in range(5)) / 5.0
    return a


def make_pair(name, B, H, W, C, L, content):
    """(x, y) fp32 [B, H, W, C] in [0, L], a different image per batch entry.  noise: independent uniform noise;
    blur: a blurred image and the same plus 2 % noise (SSIM near 1); dark: noise whose upper-left part is the constant
    0 in x and L/255 in y, so that there the denominators are near C1 C2."""
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    x = rng.random((B, H, W, C))
    if content == "noise":
        y = rng.random((B, H, W, C))
    elif content == "blur":
        x = _smooth(x)
        y = np.clip(x + 0.02 * rng.standard_normal(x.shape), 0.0, 1.0)
    elif content == "dark":
        y = np.clip(x + 0.1 * rng.standard_normal(x.shape), 0.0, 1.0)
        h, w = max(1, (2 * H) // 3), max(1, (2 * W) // 3)
        x[:, :h, :w] = 0.0
        y[:, :h, :w] = 1.0 / 255.0
    else:
        raise KeyError(content)
    return (x * L).astype(np.float32), (y * L).astype(np.float32)


def ssim_cases(tile):
    """name -> (B, H, W, C, win, L, content): the smallest shapes at which the tiling can go wrong, for the kernel's
    tile of th x tw window positions - output extents 1 x 1 and 1 x 2, every pair of {th-1, th, th+1} x {tw-1, tw,
    tw+1}, two tiles and a bit each way, the windows 3, 7, 11, 31, C in {1, 3, 4}, B in {1, 3}, L in {1, 255} and the
    three contents, rotated through the cases so that each value meets each kind of edge"""
    th, tw = tile
    cases = {}

    def add(name, oh, ow, B, C, win, L, content):
        cases[name] = (B, oh + win - 1, ow + win - 1, C, win, L, content)

    add("one_position", 1, 1, 1, 3, 11, 1.0, "noise")
    add("one_by_two", 1, 2, 3, 1, 11, 255.0, "blur")
    k = 0
    for dh in (-1, 0, 1):
        for dw in (-1, 0, 1):
            add(f"edge_{th + dh}x{tw + dw}", th + dh, tw + dw, (1, 3)[k % 2], (1, 3, 4)[k % 3], 11,
                (1.0, 255.0)[(k // 2) % 2], CONTENTS[k % 3])
            k += 1
    add("two_tiles_each_way", 2 * th + 1, 2 * tw + 3, 3, 3, 11, 1.0, "dark")
    add("win3", th + 1, tw, 1, 4, 3, 255.0, "dark")
    add("win3_one_position", 1, 1, 3, 1, 3, 1.0, "noise")
    add("win7", th, 2 * tw + 1, 3, 3, 7, 1.0, "blur")
    add("win31_one_position", 1, 1, 1, 4, 31, 1.0, "blur")
    add("win31", th + 1, tw + 2, 3, 4, 31, 255.0, "noise")
    add("win31_c1", th - 1, tw + 1, 1, 1, 31, 1.0, "dark")
    return cases


@functools.lru_cache(maxsize=None)
def ssim_case(name, tile):
    """(x, y, (ssim, map) of the reference, win, L) of ssim_cases(tile)[name]; computed once, do not modify"""
    B, H, W, C, win, L, content = ssim_cases(tile)[name]
    x, y = make_pair(name, B, H, W, C, L, content)
    for a in (x, y):
        a.setflags(write=False)
    return x, y, ssim_ref(x, y, L, win), win, L


def psnr_cases(block_pixels):
    """name -> (B, H, W, C, L): one scalar, a small odd image, one image of exactly a workgroup's share of pixels and
    one just over it (two partials in the second stage), several workgroups with a ragged last one"""
    side = int(round(block_pixels ** 0.5))
    assert side * side == block_pixels
    return {
        "one_scalar": (1, 1, 1, 1, 1.0),
        "7x5x3": (3, 7, 5, 3, 255.0),
        "one_share": (1, side, side, 4, 1.0),
        "just_over_one_share": (3, side, side + 1, 3, 1.0),
        "five_shares_ragged": (2, 2 * side + 1, 2 * side + 3, 1, 255.0),
    }


def psnr_masks(name, B, H, W):
    """[B, H, W] bool: random per batch entry; with B >= 2 entry 0 is empty and entry 1 full"""
    rng = np.random.default_rng(zlib.crc32(("mask_" + name).encode()))
    m = rng.random((B, H, W)) < 0.4
    if B >= 2:
        m[0] = False
        m[1] = True
    return m
