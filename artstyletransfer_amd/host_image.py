"""Host-side image preparation around the hot path: pyramid resize and the structured-noise
initial image (reference: neural_style_transfer.py:211-226, :249-362, :396-439).

The reference does this with OpenCV, which is absent offline; the OpenCV operators it calls are
restated here from their documented semantics (pinned by independent implementations in
tests/test_oracle_cv2.py; the driver logic around them by what the reference's own
neural_style_transfer() produced, tests/test_oracle_jobsetup.py - see DESIGN.md section 2):
  cv2.resize(..., INTER_CUBIC)   bicubic, A = -0.75, half-pixel centres, replicate border, no antialias
                                 (the rule torch's bicubic follows: torch:include/ATen/native/UpSample.h:297-309)
  cv2.Sobel(ksize=5)             separable [-1,-2,0,2,1] x [1,4,6,4,1], BORDER_REFLECT_101
  cv2.getGaussianKernel(n, s)    exp(-(i-(n-1)/2)^2 / (2 s^2)), normalised to sum 1
  cv2.GaussianBlur               separable correlation with that kernel, BORDER_REFLECT_101
This runs once per job, before the optimisation loop; it is not on the timed path."""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F
from scipy.ndimage import correlate1d

from .color_modes import PRESERVE_COLOR_MODES, check_preserve_color  # noqa: F401  (the job API's choices)

BASE_DIAMETER = 256   # neural_style_transfer.py:213


def level_size(height: int, width: int, level: int):
    """(new_height, new_width) of pyramid level `level` (neural_style_transfer.py:215-224)."""
    if height >= width:
        bw = BASE_DIAMETER
        bh = int(bw * (height / width))
    else:
        bh = BASE_DIAMETER
        bw = int(bh * (width / height))
    return bh * 2 ** level, bw * 2 ** level


def bicubic_resize(img: np.ndarray, new_height: int, new_width: int) -> np.ndarray:
    """cv2.resize(img, (new_width, new_height), interpolation=cv2.INTER_CUBIC) for float HWC images."""
    a = np.asarray(img)
    dt = a.dtype if a.dtype in (np.float32, np.float64) else np.float32
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=dt))
    squeeze = t.ndim == 2
    if squeeze:
        t = t.unsqueeze(-1)
    t = t.permute(2, 0, 1).unsqueeze(0)
    out = F.interpolate(t, size=(new_height, new_width), mode="bicubic", align_corners=False)
    out = out.squeeze(0).permute(1, 2, 0).contiguous().numpy()
    return out[..., 0] if squeeze else out


def resize_to_level(img: np.ndarray, level: int) -> np.ndarray:
    h, w = img.shape[:2]
    nh, nw = level_size(h, w, level)
    return bicubic_resize(img, nh, nw)


def gaussian_kernel(n: int, sigma: float) -> np.ndarray:
    i = np.arange(n, dtype=np.float64) - (n - 1) / 2.0
    k = np.exp(-(i * i) / (2.0 * sigma * sigma))
    return k / k.sum()


def gaussian_mask(shape, central_amplitude, peripheral_amplitude, dispersion_scale=0.5) -> np.ndarray:
    """Gaussian envelope p + g_norm * (c - p), repeated over 3 channels, float64
    (neural_style_transfer.py:396-418)."""
    rows, cols = shape[:2]
    kx = gaussian_kernel(cols, cols * dispersion_scale)
    ky = gaussian_kernel(rows, rows * dispersion_scale)
    kernel = np.outer(ky, kx)
    norm = kernel / kernel[rows // 2, cols // 2]
    mask = peripheral_amplitude + norm * (central_amplitude - peripheral_amplitude)
    return np.repeat(mask[:, :, None], 3, axis=2)


def make_style_noise(style_img: np.ndarray, targ_shape) -> np.ndarray:
    """Style pixels resized to the low-res grid and row-shuffled with the global numpy RNG
    (neural_style_transfer.py:422-439)."""
    nh, nw = targ_shape[0], targ_shape[1]
    small = bicubic_resize(style_img.copy(), nh, nw)
    vect = small.reshape(nh * nw, -1)
    return np.random.permutation(vect).reshape(targ_shape)


_SOBEL_D = np.array([-1.0, -2.0, 0.0, 2.0, 1.0])
_SOBEL_S = np.array([1.0, 4.0, 6.0, 4.0, 1.0])


def sobel5(img: np.ndarray, dx: int, dy: int) -> np.ndarray:
    a = np.asarray(img, dtype=np.float64)
    kx = _SOBEL_D if dx else _SOBEL_S
    ky = _SOBEL_D if dy else _SOBEL_S
    out = correlate1d(a, kx, axis=1, mode="mirror")
    return correlate1d(out, ky, axis=0, mode="mirror")


def gaussian_blur(img: np.ndarray, ksize: int, sigma: float) -> np.ndarray:
    k = gaussian_kernel(ksize, sigma)
    out = correlate1d(np.asarray(img, dtype=np.float64), k, axis=1, mode="mirror")
    return correlate1d(out, k, axis=0, mode="mirror")


def noise_map(style_top: np.ndarray, shape, noise_levels, central, peripheral, dispersion) -> np.ndarray:
    """Multi-granularity style noise under Gaussian envelopes (neural_style_transfer.py:265-313)."""
    nh, nw = shape[0], shape[1]
    acc = np.zeros(shape, dtype=np.float32)
    for gran, c, p, disp in zip(noise_levels, central, peripheral, dispersion):
        if gran == 0:
            acc += gaussian_mask(shape, c, p, disp)
            continue
        if gran > 0:
            if nh <= nw:
                dh, dw = gran, nw * gran // nh
            else:
                dw, dh = gran, nh * gran // nw
        else:
            dw, dh = nw // (-gran), nh // (-gran)
        low = make_style_noise(style_top, (dh, dw, shape[2]))
        hi = bicubic_resize(low, nh, nw)
        acc += hi * gaussian_mask(hi.shape, c, p, disp)
    return acc


def gradient_weight(content_top: np.ndarray, noise_factor: float) -> np.ndarray:
    """a*noise_factor/(a + |sobel|) with a = 5 (neural_style_transfer.py:331-343)."""
    sx = np.absolute(sobel5(content_top, 1, 0))
    sy = np.absolute(sobel5(content_top, 0, 1))
    mag = np.clip(np.sqrt(sx * sx + sy * sy), 0.0, 100)
    mag = gaussian_blur(mag, 101, 0.2)
    a = 5.0
    return a * noise_factor / (a + mag)


def initial_image(init_method: str, content_img: np.ndarray, style_img: np.ndarray, content_top: np.ndarray,
                  style_top: np.ndarray, top_level: int, noise_factor, noise_levels, central, peripheral, dispersion):
    """(init image float32 HWC, name tag) per neural_style_transfer.py:265-362."""
    noise = noise_map(style_top, content_top.shape, noise_levels, central, peripheral, dispersion)
    weight = gradient_weight(content_top, noise_factor)
    if init_method == "random":
        return noise * 0.5, "random"
    if init_method == "content+noise":
        base = resize_to_level(content_img, top_level)
        return ((1.0 - weight) * base + weight * noise).astype(np.float32), "content"
    return resize_to_level(style_img, top_level), "style"


# ---- colour preservation (Gatys, Bethge, Hertzmann & Shechtman, "Preserving Color in Neural Artistic Style Transfer",
# 2016): the fp64 restatement of image_ops.hip's set-up kernels (nst_color_stats, nst_color_transfer_matrix,
# nst_color_affine, nst_luminance, nst_luminance_recombine); images HWC float RGB in [0,1]
LUMA = np.array([0.299, 0.587, 0.114])
YIQ = np.array([[0.299, 0.587, 0.114],
                [0.595716, -0.274453, -0.321263],
                [0.211456, -0.522591, 0.311135]])
YIQ_INV = np.linalg.inv(YIQ)


def color_stats(img: np.ndarray):
    """(mean (3,), population covariance (3,3)) of the pixels of an HWC RGB image, fp64."""
    p = np.asarray(img, dtype=np.float64).reshape(-1, 3)
    mu = p.mean(axis=0)
    d = p - mu
    return mu, d.T @ d / p.shape[0]


def color_transfer_matrix(stats_c, stats_s):
    """(A, b) with A = Sigma_c^{1/2} Sigma_s^{-1/2} (symmetric square roots; style eigenvalues clamped below at 1e-10) and
    b = mu_c - A mu_s: A p + b has the content's mean and covariance."""
    (mu_c, cov_c), (mu_s, cov_s) = stats_c, stats_s
    ec, vc = np.linalg.eigh(np.asarray(cov_c, dtype=np.float64))
    es, vs = np.linalg.eigh(np.asarray(cov_s, dtype=np.float64))
    root_c = (vc * np.sqrt(np.maximum(ec, 0.0))) @ vc.T
    inv_root_s = (vs / np.sqrt(np.maximum(es, 1e-10))) @ vs.T
    A = root_c @ inv_root_s
    return A, np.asarray(mu_c, dtype=np.float64) - A @ np.asarray(mu_s, dtype=np.float64)


def color_affine(img: np.ndarray, A: np.ndarray, b: np.ndarray) -> np.ndarray:
    """Every pixel p -> A p + b (fp64, stored float32, not clipped)."""
    p = np.asarray(img, dtype=np.float64)
    return (p @ np.asarray(A, dtype=np.float64).T + b).astype(np.float32)


def luminance_params(stats_c, stats_s):
    """(alpha, beta) matching the style's luminance mean and deviation to the content's: alpha = sigma_Yc / sigma_Ys
    (0 for a flat style, sigma_Ys < 1e-12), beta = mu_Yc - alpha mu_Ys."""
    (mu_c, cov_c), (mu_s, cov_s) = stats_c, stats_s
    m_c, m_s = float(LUMA @ mu_c), float(LUMA @ mu_s)
    s_c = float(np.sqrt(max(LUMA @ cov_c @ LUMA, 0.0)))
    s_s = float(np.sqrt(max(LUMA @ cov_s @ LUMA, 0.0)))
    alpha = s_c / s_s if s_s >= 1e-12 else 0.0
    return alpha, m_c - alpha * m_s


def luminance(img: np.ndarray, alpha: float = 1.0, beta: float = 0.0) -> np.ndarray:
    """(1,h,w) float32 255 (alpha Y + beta), Y = 0.299 R + 0.587 G + 0.114 B."""
    y = np.asarray(img, dtype=np.float64) @ LUMA
    return (255.0 * (alpha * y + beta)).astype(np.float32)[None]


def luminance_recombine(u: np.ndarray, content: np.ndarray) -> np.ndarray:
    """HWC float32 YIQ^-1 (u / 255, I(content), Q(content)), not clipped: the RGB image of a luminance job."""
    c = np.asarray(content, dtype=np.float64)
    yiq = c @ YIQ.T
    yiq[..., 0] = np.asarray(u, dtype=np.float64).reshape(c.shape[:2]) / 255.0
    return (yiq @ YIQ_INV.T).astype(np.float32)
