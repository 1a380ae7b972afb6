"""Thin Python handle on the C ABI: device buffers are torch CUDA tensors (plumbing only), every
computation happens in libnst_hip.so."""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from . import taps as _taps
from .pooling_modes import check_pooling
from . import style_modes as _style
from . import regions as _regions
from . import gram_modes as _gram
from . import moment_modes as _mom
from . import laplacian_modes as _lap
from . import matting_modes as _mat
from . import flow_modes as _flow
from . import mrf_modes as _mrf
from . import hist_modes as _hist
from . import remd_modes as _remd
from . import selfsim_modes as _selfsim
from . import xcorr_modes as _xcorr
from ._lib import NST_LOSS_ROW, NstError, StepInfo

TAP_CHANNELS = (64, 128, 256, 512, 512, 512)
TAP_SCALE = (0, 1, 2, 3, 3, 4)
DEFAULT_TAPS = (_taps.DEFAULT_CONTENT_INDEX, _taps.DEFAULT_STYLE_INDICES, True)


# The job settings a StyleEngine caches: (attribute, method that reads the context's setting, method that undoes the setting,
# whether nst_job_configure clears it), in the order reset_job_settings undoes them.
_JOB_SETTINGS = (
    ("layer_weights", "style_weights", "reset_style_weights", False),
    ("taps", None, "reset_taps", False),                      # (set_taps caches what it set: no reader)
    ("channels", "_channels", "reset_color", False),
    ("pooling", "_pooling", "reset_pooling", False),
    ("laplacian", "laplacian_setting", "reset_laplacian", True),
    ("gram_shift", "gram_shift_setting", "reset_gram_shift", True),
    ("matting", "matting_setting", "reset_matting", True),
    ("moment_loss", "moments_setting", "reset_moments", True),
)
_READER = {attr: reader for attr, reader, _, _ in _JOB_SETTINGS}


def _ptr(t: Optional[torch.Tensor]):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _stream(device) -> C.c_void_p:
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _chk_dev(t: torch.Tensor, device, shape=None):
    if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
        raise NstError("expected a contiguous float32 CUDA tensor")
    if t.device != device:
        raise NstError(f"tensor is on {t.device}, context on {device}")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise NstError(f"expected shape {tuple(shape)}, got {tuple(t.shape)}")


def flow_workspace(h: int, w: int, scales: int = 0) -> Tuple[int, int]:
    """(floats of the workspace nst_flow_estimate needs for two (h,w) planes, pyramid scales it uses) (nst_flow_workspace): a
    pure function of the library, no GPU.  ValueError for h or w < 1 and scales outside 0 .. NST_MAX_FLOW_SCALES."""
    floats, used = C.c_size_t(), C.c_int()
    if _lib.load().nst_flow_workspace(int(h), int(w), int(scales), C.byref(floats), C.byref(used)) != _lib.NST_OK:
        raise ValueError(f"no flow workspace for {h}x{w} planes and scales={scales}")
    return floats.value, used.value


def flow_tvl1_workspace(h: int, w: int, scales: int = 0) -> Tuple[int, int]:
    """flow_workspace for nst_flow_tvl1_estimate (nst_flow_tvl1_workspace): that workspace plus two copies of the duals."""
    floats, used = C.c_size_t(), C.c_int()
    if _lib.load().nst_flow_tvl1_workspace(int(h), int(w), int(scales), C.byref(floats), C.byref(used)) != _lib.NST_OK:
        raise ValueError(f"no TV-L1 flow workspace for {h}x{w} planes and scales={scales}")
    return floats.value, used.value


class StyleEngine:
    """One nst_ctx: VGG19 weights on one GPU + the pyramid workspace of one job."""

    def __init__(self, weights: Sequence[Tuple[torch.Tensor, torch.Tensor]], device: int | str | torch.device = 0,
                 conv_mode: Optional[str] = None, batched: Optional[bool] = None, single_stream: Optional[bool] = None,
                 use_graph: Optional[bool] = None, h2_band_rows: Optional[int] = None, lbfgs_gram: Optional[bool] = None,
                 h2_mfma16: Optional[bool] = None, h2_wg256: Optional[bool] = None,
                 h2_tile_rows: Optional[int] = None, gram_overlap: Optional[bool] = None,
                 h2_persist: Optional[bool] = None, level_split: Optional[bool] = None,
                 h2_winograd: Optional[bool] = None, keep_all_maps: Optional[bool] = None,
                 forward_pack: Optional[bool] = None, gram_pack: Optional[bool] = None,
                 h2_direct_weights: Optional[bool] = None):
        """Options (nst_options): None = environment variable (NST_CONV, NST_BATCH, NST_SINGLE_STREAM, NST_GRAPH,
        NST_H2_BAND_ROWS, NST_LBFGS_GRAM, NST_H2_MFMA16; read once, here) and otherwise the default (f16x2, batched, ...).
        keep_all_maps (nst_ctx_set_keep_all_maps; None = env NST_KEEP_ALL_MAPS, default off): every batched forward launch
        stores its full-resolution map, also the four that nothing reads - same results, the A/B twin of the elision.
        forward_pack (nst_ctx_set_forward_pack; None = env NST_FORWARD_PACK, default on): False = the forward half's front and
        loss terms launched per pyramid level, S also written in bf16 pieces - same results, the A/B twin of the packing.
        gram_pack (nst_ctx_set_gram_pack; None = env NST_GRAM_PACK, default on): False = the Gram partial kernels compute every
        block of a diagonal tile and a batch launches once per tile shape - same results, the A/B twin of the packed Gram pass.
        h2_direct_weights (nst_ctx_set_h2_direct_weights; None = env NST_H2_DIRECT_WEIGHTS, default on): False = the forward
        launches of conv1_2, conv2_1, conv2_2 and conv3_1 stage their weight slices through LDS instead of reading fragments
        from L2 - same results, the A/B twin of the one-barrier-per-chunk K loop.  True = both kernel shapes; an int is the
        setter's mask (1 = conv1_2's shape, 2 = the shape of the other three)."""
        self.lib = _lib.load()
        if not torch.cuda.is_available():
            raise NstError("no GPU visible: the style-transfer hot path runs only on the HIP device")
        self.device = torch.device(device if not isinstance(device, int) else f"cuda:{device}")
        if self.device.type != "cuda":
            raise NstError("StyleEngine needs a cuda (HIP) device; there is no CPU fallback")
        idx = self.device.index if self.device.index is not None else torch.cuda.current_device()
        self.device = torch.device("cuda", idx)
        if len(weights) != _lib.NST_VGG19_CONVS:
            raise NstError("expected 13 (weight, bias) pairs conv1_1..conv5_1")
        ws = [np.ascontiguousarray(w.detach().cpu().numpy(), dtype=np.float32) for w, _ in weights]
        bs = [np.ascontiguousarray(b.detach().cpu().numpy(), dtype=np.float32) for _, b in weights]
        wp = (C.c_void_p * 13)(*[a.ctypes.data for a in ws])
        bp = (C.c_void_p * 13)(*[a.ctypes.data for a in bs])
        opts = _lib.Options()
        self.lib.nst_options_default(C.byref(opts))
        if conv_mode is not None:
            if conv_mode not in _lib.CONV_MODES:
                raise NstError(f"conv_mode must be one of {sorted(_lib.CONV_MODES)}")
            opts.conv_mode = _lib.CONV_MODES[conv_mode]
        for name, val in (("batched", batched), ("single_stream", single_stream), ("use_graph", use_graph),
                          ("h2_band_rows", h2_band_rows), ("lbfgs_gram", lbfgs_gram), ("h2_mfma16", h2_mfma16),
                          ("h2_wg256", h2_wg256), ("h2_tile_rows", h2_tile_rows),
                          ("gram_overlap", gram_overlap), ("h2_persist", h2_persist), ("level_split", level_split), ("h2_winograd", h2_winograd)):
            if val is not None:
                setattr(opts, name, int(val))
        ctx = C.c_void_p()
        _lib.check(None, self.lib.nst_ctx_create_ex(idx, wp, bp, C.byref(opts), C.byref(ctx)), "nst_ctx_create_ex")
        self.ctx = ctx
        if keep_all_maps is not None:
            _lib.check(self.ctx, self.lib.nst_ctx_set_keep_all_maps(self.ctx, int(bool(keep_all_maps))), "nst_ctx_set_keep_all_maps")
        if forward_pack is not None:
            _lib.check(self.ctx, self.lib.nst_ctx_set_forward_pack(self.ctx, int(bool(forward_pack))), "nst_ctx_set_forward_pack")
        if gram_pack is not None:
            _lib.check(self.ctx, self.lib.nst_ctx_set_gram_pack(self.ctx, int(bool(gram_pack))), "nst_ctx_set_gram_pack")
        if h2_direct_weights is not None:
            _lib.check(self.ctx, self.lib.nst_ctx_set_h2_direct_weights(
                self.ctx, 3 if h2_direct_weights is True else int(h2_direct_weights)),
                       "nst_ctx_set_h2_direct_weights")
        self.weights_id = id(weights)          # which weight set this context carries (neural_nets' engine pool)
        self.levels = 0
        self.shape = None
        self.taps = DEFAULT_TAPS                 # (content index, style indices, use_relu): set_taps
        self.channels = 3                        # 1 under set_color("luminance")
        self.pooling = "max"                     # "avg" under set_pooling("avg")
        self.layer_weights = _style.UNIT_WEIGHTS # set_style_weights
        self.laplacian = None                    # (pools, weights) under set_laplacian
        self.matting = None                      # (gamma, epsilon) under set_matting
        self.gram_shift = None                   # (shift[6], center_mask) under set_gram_shift
        self.moment_loss = None                  # (mean_w[6], std_w[6], epsilon) under set_moments

    def close(self):
        if getattr(self, "ctx", None):
            self.lib.nst_ctx_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- job ------------------------------------------------------------------------------------
    def configure(self, levels_num: int, H0: int, W0: int) -> None:
        _lib.check(self.ctx, self.lib.nst_job_configure(self.ctx, levels_num, H0, W0), "nst_job_configure")
        self.levels = levels_num
        self.shape = (H0, W0)
        for attr, _, _, cleared in _JOB_SETTINGS:   # (nst_job_configure clears the settings of the loss terms)
            if cleared:
                setattr(self, attr, None)

    def _set_native(self, attr: str, fn: str, *args) -> None:
        """Call the native setter `fn`, then - whether it succeeded or not - re-read the context's setting into the cached
        attribute `attr`."""
        try:
            _lib.check(self.ctx, getattr(self.lib, fn)(self.ctx, *args), fn)
        finally:
            setattr(self, attr, getattr(self, _READER[attr])())

    def reset_job_settings(self) -> None:
        """Every job setting back to the reference's, if it was changed: unit style weights (before the taps: a style set
        needs a map with a positive weight), the default taps, RGB, max pooling, no Laplacian, Gram shift, matting or
        moment term."""
        for _, _, reset, _ in _JOB_SETTINGS:
            getattr(self, reset)()

    def set_taps(self, content_index, style_indices, use_relu: bool = True) -> None:
        """The feature maps the losses read (nst_job_set_taps): a content index and style indices of Vgg19.layer_names
        (0..5, or names of the `use_relu` flavour; order and repeats of the style list do not matter).  Drops the
        targets of every configured level: call set_targets again.  ValueError for an invalid choice."""
        content, style = _taps.normalize_taps(content_index, style_indices, use_relu)
        _lib.check(self.ctx, self.lib.nst_job_set_taps(self.ctx, content, _taps.style_mask(style), int(use_relu)),
                   "nst_job_set_taps")
        self.taps = (content, style, bool(use_relu))

    def reset_taps(self) -> None:
        """Back to the reference's taps (content 4, style 0, 1, 2, 3, 5, post-ReLU), if they were changed."""
        if self.taps != DEFAULT_TAPS:
            self.set_taps(*DEFAULT_TAPS)

    def set_color(self, mode) -> None:
        """Channel count of the optimised image (nst_job_set_color): "rgb" (or None) = prepared RGB (1,3,H,W), "luminance"
        = one plane u = 255 Y (1,1,H,W) that the network sees as u - mean_c.  Drops the targets of every configured
        level: call set_targets again."""
        if mode not in (None, "rgb", "luminance"):
            raise ValueError(f"colour mode must be 'rgb' or 'luminance', not {mode!r}")
        self._set_native("channels", "nst_job_set_color", _lib.NST_COLOR_LUMINANCE if mode == "luminance" else _lib.NST_COLOR_RGB)

    def _channels(self) -> int:
        return 1 if self.lib.nst_job_color(self.ctx) == _lib.NST_COLOR_LUMINANCE else 3

    def reset_color(self) -> None:
        """Back to RGB, if the colour mode was changed."""
        if self.channels != 3:
            self.set_color("rgb")

    def set_pooling(self, mode) -> None:
        """Pooling of the feature network (nst_job_set_pooling): "max" = torchvision's vgg19, "avg" = every 2x2 max-pool
        replaced by a 2x2 average pool (Gatys et al. 2016).  Drops the targets of every configured level: call
        set_targets again.  ValueError for any other value."""
        check_pooling(mode)
        self._set_native("pooling", "nst_job_set_pooling", _lib.NST_POOL_AVG if mode == "avg" else _lib.NST_POOL_MAX)

    def _pooling(self) -> str:
        return "avg" if self.lib.nst_job_pooling(self.ctx) == _lib.NST_POOL_AVG else "max"

    def reset_pooling(self) -> None:
        """Back to max pooling, if the mode was changed."""
        if self.pooling != "max":
            self.set_pooling("max")

    def set_style_weights(self, w) -> None:
        """Per-layer style weights (nst_job_set_style_weights): six numbers >= 0, one per map of Vgg19.layer_names; the
        style term becomes (sum_i w_i MSE_i) / nstyle.  Keeps the targets.  ValueError for a wrong length, a negative or
        non-finite entry, or when no map of the current style set has a positive weight."""
        w = _style.check_style_layer_weights(w, style_indices=self.taps[1])
        self._set_native("layer_weights", "nst_job_set_style_weights", (C.c_float * _style.NUM_MAPS)(*w))

    def style_weights(self) -> Tuple[float, ...]:
        """The context's six style layer weights (nst_job_style_weights)."""
        arr = (C.c_float * _style.NUM_MAPS)()
        _lib.check(self.ctx, self.lib.nst_job_style_weights(self.ctx, arr), "nst_job_style_weights")
        return tuple(float(v) for v in arr)

    def reset_style_weights(self) -> None:
        """Back to w = 1 on every map, if the weights were changed."""
        if self.layer_weights != _style.UNIT_WEIGHTS:
            self.set_style_weights(_style.UNIT_WEIGHTS)

    def set_laplacian(self, pools, weights) -> None:
        """The Laplacian loss of the job (nst_job_set_laplacian; Li et al. 2017): pool sizes (integers 1..32, distinct) and
        their weights gamma >= 0, each a number or a sequence of up to four; the level total gains sum_k gamma_k lap_k.
        All-zero weights switch the term off.  Needs a configured job; drops the targets of every level: call set_targets
        again.  ValueError (before the context is touched) for a malformed setting or a level too small for a pool size."""
        entries = _lap.normalize_laplacian(weights, pools)
        if entries is None:
            self.reset_laplacian()
            return
        if not self.levels:
            raise NstError("set_laplacian needs a configured job (configure first)")
        _lap.check_levels(entries[0], self.levels, *self.shape)
        k = len(entries[0])
        pool = (C.c_int * k)(*entries[0])
        gamma = (C.c_float * k)(*entries[1])
        self._set_native("laplacian", "nst_job_set_laplacian", k, pool, gamma)

    def laplacian_setting(self):
        """The context's Laplacian entries as (pools, weights), or None when the term is off (nst_job_laplacian)."""
        k = C.c_int()
        pool = (C.c_int * _lib.NST_MAX_LAPLACIAN)()
        gamma = (C.c_float * _lib.NST_MAX_LAPLACIAN)()
        _lib.check(self.ctx, self.lib.nst_job_laplacian(self.ctx, C.byref(k), pool, gamma), "nst_job_laplacian")
        if k.value == 0:
            return None
        return tuple(int(v) for v in pool[:k.value]), tuple(float(v) for v in gamma[:k.value])

    def reset_laplacian(self) -> None:
        """The Laplacian term off, if it was set (drops the targets then, as set_laplacian does)."""
        if self.laplacian is not None:
            self._set_native("laplacian", "nst_job_set_laplacian", 0, None, None)

    def laplacian_losses(self) -> torch.Tensor:
        """(levels, 4) device tensor: the unweighted lap_k of the last closure per level and entry
        (nst_job_laplacian_losses); zeros for levels outside the last level mask and for unused entries."""
        out = torch.empty((self.levels, _lib.NST_MAX_LAPLACIAN), dtype=torch.float32, device=self.device)
        _lib.check(self.ctx, self.lib.nst_job_laplacian_losses(self.ctx, _ptr(out), _stream(self.device)),
                   "nst_job_laplacian_losses")
        return out

    def set_matting(self, gamma, epsilon=_mat.DEFAULT_EPSILON) -> None:
        """The matting term of the job (nst_job_set_matting; Luan et al. 2017): the level total gains gamma * mat, the
        quadratic form of the matting Laplacian of the level's content on the level image.  gamma None or 0 switches the
        term off.  Needs a configured job; drops the targets of every level: call set_targets again.  ValueError (before
        the context is touched) for a malformed setting or a level smaller than 3x3."""
        setting = _mat.normalize_matting(gamma, epsilon)
        if setting is None:
            self.reset_matting()
            return
        if not self.levels:
            raise NstError("set_matting needs a configured job (configure first)")
        _mat.check_levels(self.levels, *self.shape)
        self._set_native("matting", "nst_job_set_matting", setting[0], setting[1])

    def matting_setting(self):
        """The context's matting term as (gamma, epsilon), or None when it is off (nst_job_matting)."""
        gamma, eps = C.c_float(), C.c_double()
        _lib.check(self.ctx, self.lib.nst_job_matting(self.ctx, C.byref(gamma), C.byref(eps)), "nst_job_matting")
        return (float(gamma.value), float(eps.value)) if gamma.value > 0 else None

    def reset_matting(self) -> None:
        """The matting term off, if it was set (drops the targets then, as set_matting does)."""
        if self.matting is not None:
            self._set_native("matting", "nst_job_set_matting", 0.0, self.matting[1])

    def matting_losses(self) -> torch.Tensor:
        """(levels,) device tensor: the unweighted mat of the last closure per level (nst_job_matting_losses); zeros for
        levels outside the last level mask and while the term is off."""
        out = torch.empty((self.levels,), dtype=torch.float32, device=self.device)
        _lib.check(self.ctx, self.lib.nst_job_matting_losses(self.ctx, _ptr(out), _stream(self.device)),
                   "nst_job_matting_losses")
        return out

    def set_gram_shift(self, shift, center_mask: int = 0) -> None:
        """The Gram statistic of the job (nst_job_set_gram_shift): `shift` - None, a number, "mean", six entries or a dict, as
        gram_modes.normalize_gram_shift takes them, the explicit form being six floats with `center_mask`, the bit set of the
        centred maps (whose shift is 0).  G = (F + o)^T (F + o) / (C N) with o the map's constant shift or minus its own
        channel means.  All zeros with an empty mask: the plain Gram.  Needs a configured job, the f16x2 arithmetic and no
        guided level; drops the targets of every level: call set_targets again.  ValueError (before the context is touched)
        for a malformed setting."""
        setting = _gram.normalize_gram_shift(shift)
        mask = int(center_mask)
        if mask < 0 or mask >> _gram.NUM_MAPS:
            raise ValueError(f"center_mask must be a set of bits 0..{_gram.NUM_MAPS - 1}, got {center_mask!r}")
        if mask:
            s6, m0 = setting if setting is not None else ((0.0,) * _gram.NUM_MAPS, 0)
            if any(s6[i] != 0.0 for i in range(_gram.NUM_MAPS) if (mask >> i) & 1):
                raise ValueError("a centred map takes no constant shift: its entry must be 0")
            setting = (s6, m0 | mask)
        if setting is None:
            self.reset_gram_shift()
            return
        if not self.levels:
            raise NstError("set_gram_shift needs a configured job (configure first)")
        self._set_native("gram_shift", "nst_job_set_gram_shift", (C.c_float * _gram.NUM_MAPS)(*setting[0]), setting[1])

    def gram_shift_setting(self):
        """The context's Gram shift as (shift[6], center_mask), or None when it is off (nst_job_gram_shift)."""
        arr = (C.c_float * _gram.NUM_MAPS)()
        mask = C.c_uint(0)
        _lib.check(self.ctx, self.lib.nst_job_gram_shift(self.ctx, arr, C.byref(mask)), "nst_job_gram_shift")
        shift = tuple(float(v) for v in arr)
        if mask.value == 0 and all(v == 0.0 for v in shift):
            return None
        return shift, int(mask.value)

    def reset_gram_shift(self) -> None:
        """The plain Gram statistic again, if a shift was set (drops the targets then, as set_gram_shift does)."""
        if self.gram_shift is not None:
            self._set_native("gram_shift", "nst_job_set_gram_shift", (C.c_float * _gram.NUM_MAPS)(), 0)

    def level_gram_offsets(self, level: int, slot: int) -> torch.Tensor:
        """(C,) device tensor: the offsets o that the last closure of `level` used for style slot `slot` (the slots are the
        style maps of the current taps in ascending order; nst_level_gram_offsets)."""
        style = self.taps[1]
        if not 0 <= slot < len(style):
            raise ValueError(f"slot {slot} is outside the {len(style)} style maps of the current taps")
        c = (64, 128, 256, 512, 512, 512)[style[slot]]      # channels of the six maps of Vgg19.layer_names
        out = torch.empty((c,), dtype=torch.float32, device=self.device)
        _lib.check(self.ctx, self.lib.nst_level_gram_offsets(self.ctx, level, slot, _ptr(out), _stream(self.device)),
                   "nst_level_gram_offsets")
        return out

    def set_moments(self, mean_w, std_w=None, epsilon=_mom.DEFAULT_EPSILON) -> None:
        """The moment loss of the job (nst_job_set_moments; Li et al. 2017, Huang & Belongie 2017): the level total gains
        sum_i (mean_w[i] mean_i + std_w[i] std_i), the mean squared differences of the channel means and of the channel
        deviations sigma = sqrt(var + epsilon) of style map i from the style's.  `mean_w`, `std_w`: each None or 0, a number
        (that weight on every style map of the current taps), six numbers by map index of Vgg19.layer_names, or a dict
        {map index or name: number}.  All zeros: off.  Needs a configured job, the f16x2 arithmetic and no guided level;
        drops the targets of every level: call set_targets again.  ValueError (before the context is touched) for a
        malformed setting or a positive weight on a map that is not a style map of the current taps."""
        setting = _mom.check_setting(mean_w, std_w, epsilon, style_indices=getattr(self, "taps", DEFAULT_TAPS)[1])
        if setting is None:
            self.reset_moments()
            return
        if not self.levels:
            raise NstError("set_moments needs a configured job (configure first)")
        wm = (C.c_float * _mom.NUM_MAPS)(*setting[0])
        ws = (C.c_float * _mom.NUM_MAPS)(*setting[1])
        self._set_native("moment_loss", "nst_job_set_moments", wm, ws, setting[2])

    def moments_setting(self):
        """The context's moment loss as (mean_w[6], std_w[6], epsilon), or None when it is off (nst_job_moments)."""
        wm = (C.c_float * _mom.NUM_MAPS)()
        ws = (C.c_float * _mom.NUM_MAPS)()
        eps = C.c_float()
        _lib.check(self.ctx, self.lib.nst_job_moments(self.ctx, wm, ws, C.byref(eps)), "nst_job_moments")
        mean_w, std_w = tuple(float(v) for v in wm), tuple(float(v) for v in ws)
        if all(v == 0.0 for v in mean_w + std_w):
            return None
        return mean_w, std_w, float(eps.value)

    def reset_moments(self) -> None:
        """The moment loss off, if it was set (drops the targets then, as set_moments does)."""
        if self.moment_loss is not None:
            zeros = (C.c_float * _mom.NUM_MAPS)()
            self._set_native("moment_loss", "nst_job_set_moments", zeros, zeros, self.moment_loss[2])

    def moment_losses(self) -> torch.Tensor:
        """(levels, 6, 2) device tensor: the unweighted (mean_i, std_i) of the last closure per level and map index
        (nst_job_moment_losses); zeros for maps without the term, levels outside the last level mask and while it is off."""
        out = torch.empty((self.levels, _mom.NUM_MAPS, 2), dtype=torch.float32, device=self.device)
        _lib.check(self.ctx, self.lib.nst_job_moment_losses(self.ctx, _ptr(out), _stream(self.device)), "nst_job_moment_losses")
        return out

    def release_job(self) -> None:
        """Give the job's pyramid workspace back (4.7 GB at L=2) and keep the context with its uploaded weights: what an
        engine waiting in neural_nets' pool holds is the smallest job nst_job_configure accepts."""
        self.configure(1, 16, 16)

    def level_shape(self, level: int) -> Tuple[int, int]:
        h, w = self.shape
        return h >> level, w >> level

    def set_targets(self, level: int, content: torch.Tensor, style: torch.Tensor) -> None:
        h, w = self.level_shape(level)
        ch = self.channels
        if content.numel() != ch * h * w or style.numel() != ch * style.shape[-2] * style.shape[-1]:
            raise NstError(f"targets must have {ch} channel(s) in this colour mode")
        content = content.contiguous().reshape(ch, h, w)
        _chk_dev(content, self.device)
        style = style.contiguous().reshape(ch, style.shape[-2], style.shape[-1])
        _chk_dev(style, self.device)
        _lib.check(self.ctx, self.lib.nst_level_set_targets(self.ctx, level, _ptr(content), _ptr(style),
                                                            style.shape[1], style.shape[2], _stream(self.device)),
                   "nst_level_set_targets")

    def set_targets_blend(self, level: int, content: torch.Tensor, styles: Sequence[torch.Tensor], blend) -> None:
        """Targets of one level with the style Gram targets blended from K style images, each of its own size
        (nst_level_set_targets_blend).  blend: K numbers (the same weight on every map) or a K x 6 array B[k][i] >= 0, the
        weight of image k on map i; the target of map i is sum_k B[k][i] G_i(style_k) / sum_k B[k][i].  ValueError for a
        malformed blend, K outside 1..8 or a map of the style set with an all-zero column."""
        h, w = self.level_shape(level)
        ch = self.channels
        styles = list(styles)
        rows = _style.check_style_blend(blend, len(styles), style_indices=self.taps[1])
        k = len(styles)
        if content.numel() != ch * h * w or any(s.numel() != ch * s.shape[-2] * s.shape[-1] for s in styles):
            raise NstError(f"targets must have {ch} channel(s) in this colour mode")
        content = content.contiguous().reshape(ch, h, w)
        _chk_dev(content, self.device)
        styles = [s.contiguous().reshape(ch, s.shape[-2], s.shape[-1]) for s in styles]
        for s in styles:
            _chk_dev(s, self.device)
        ptrs = (C.c_void_p * k)(*[s.data_ptr() for s in styles])
        hs = (C.c_int * k)(*[s.shape[1] for s in styles])
        ws = (C.c_int * k)(*[s.shape[2] for s in styles])
        flat = (C.c_float * (k * _style.NUM_MAPS))(*[v for row in rows for v in row])
        _lib.check(self.ctx, self.lib.nst_level_set_targets_blend(self.ctx, level, _ptr(content), k, ptrs, hs, ws, flat,
                                                                  _stream(self.device)), "nst_level_set_targets_blend")

    # ---- spatial control (nst_level_set_guidance; regions.py is the host side) ---------------------------
    def set_guidance(self, level: int, planes: Optional[torch.Tensor], weights=None) -> None:
        """Guidance planes of one level (nst_level_set_guidance): a device (R,h,w) float32 tensor in [0,1] of the level's
        size, 1 <= R <= 4, and R region weights >= 0 (None: ones).  planes = None clears the level's guidance.  The
        guided targets of another R become invalid: set_targets_guided again.  ValueError for weights that do not fit;
        NstError (NST_E_ARG) for values outside [0,1] or a region with a mass below 1 on a map in use, (NST_E_STATE) in
        the bf16x3 / f32 arithmetic."""
        if planes is None:
            _lib.check(self.ctx, self.lib.nst_level_set_guidance(self.ctx, level, 0, None, None, _stream(self.device)),
                       "nst_level_set_guidance")
            return
        h, w = self.level_shape(level)
        if planes.dim() != 3 or tuple(planes.shape[1:]) != (h, w):
            raise NstError(f"guidance planes of level {level} must have shape (R,{h},{w}), got {tuple(planes.shape)}")
        r = planes.shape[0]
        lam = None
        if weights is not None:
            lam = (C.c_float * max(r, 1))(*_regions.check_region_weights(weights, r))
        planes = planes.contiguous()
        _chk_dev(planes, self.device)
        _lib.check(self.ctx, self.lib.nst_level_set_guidance(self.ctx, level, r, _ptr(planes), lam, _stream(self.device)),
                   "nst_level_set_guidance")

    def clear_guidance(self) -> None:
        """No guidance on any configured level."""
        for level in range(self.levels):
            self.set_guidance(level, None)

    def set_targets_guided(self, level: int, content: torch.Tensor, style: torch.Tensor, style_planes: torch.Tensor) -> None:
        """The level's content target and the guided Gram targets of the R regions of its guidance
        (nst_level_set_targets_guided): style_planes is a device (R,hs,ws) float32 tensor in [0,1] of the style image's
        size.  set_guidance first."""
        h, w = self.level_shape(level)
        ch = self.channels
        if content.numel() != ch * h * w or style.numel() != ch * style.shape[-2] * style.shape[-1]:
            raise NstError(f"targets must have {ch} channel(s) in this colour mode")
        content = content.contiguous().reshape(ch, h, w)
        _chk_dev(content, self.device)
        style = style.contiguous().reshape(ch, style.shape[-2], style.shape[-1])
        _chk_dev(style, self.device)
        r = self.guidance(level)[0]
        if style_planes.dim() != 3 or tuple(style_planes.shape) != (r, style.shape[1], style.shape[2]):
            raise NstError(f"style planes must have shape ({r},{style.shape[1]},{style.shape[2]}), got {tuple(style_planes.shape)}")
        style_planes = style_planes.contiguous()
        _chk_dev(style_planes, self.device)
        _lib.check(self.ctx, self.lib.nst_level_set_targets_guided(self.ctx, level, _ptr(content), _ptr(style), style.shape[1],
                                                                   style.shape[2], _ptr(style_planes), _stream(self.device)),
                   "nst_level_set_targets_guided")

    def guidance(self, level: int):
        """(R, region weights (R,), masses (5,R) float64: n_r of the five network scales) of a level (nst_level_guidance);
        R = 0: the level is not guided."""
        r = C.c_int()
        lam = (C.c_float * _regions.MAX_REGIONS)()
        mass = (C.c_double * (_regions.NUM_SCALES * _regions.MAX_REGIONS))()
        _lib.check(self.ctx, self.lib.nst_level_guidance(self.ctx, level, C.byref(r), lam, mass), "nst_level_guidance")
        m = np.array(list(mass), dtype=np.float64).reshape(_regions.NUM_SCALES, _regions.MAX_REGIONS)
        return r.value, tuple(float(v) for v in lam[:r.value]), m[:, :r.value].copy()

    def guidance_planes(self, level: int, scale: int) -> torch.Tensor:
        """The (R, h >> scale, w >> scale) guidance of one network scale of a guided level (nst_level_guidance_planes)."""
        h, w = self.level_shape(level)
        r = self.guidance(level)[0]
        out = torch.empty((r, h >> scale, w >> scale), dtype=torch.float32, device=self.device)
        _lib.check(self.ctx, self.lib.nst_level_guidance_planes(self.ctx, level, scale, _ptr(out), _stream(self.device)),
                   "nst_level_guidance_planes")
        return out

    # ---- temporal consistency (nst_level_set_anchor; video.py is the driver) -----------------------------
    def set_anchor(self, level: int, anchor: Optional[torch.Tensor], weights: Optional[torch.Tensor] = None, *, gamma) -> None:
        """The temporal term of one level (nst_level_set_anchor; Ruder et al. 2016): the level total gains gamma * tmp, the
        mean over channels and pixels of weights(p) (y - anchor)^2.  anchor: a device float32 tensor of the level image's
        size ((C,h,w), any leading ones; C = 3, or 1 in luminance mode), weights: (h,w) in [0,1] or None for ones; both are
        copied.  Data of the job, not a setting: configure() drops it.  anchor None or gamma 0 clears the level's term."""
        gamma = float(gamma)
        if anchor is None:
            _lib.check(self.ctx, self.lib.nst_level_set_anchor(self.ctx, int(level), None, None, 0.0, _stream(self.device)),
                       "nst_level_set_anchor")
            return
        if not 0 <= level < self.levels:
            raise NstError(f"level {level} is not configured")
        h, w = self.level_shape(level)
        ch = self.channels
        if anchor.numel() != ch * h * w or tuple(anchor.shape[-2:]) != (h, w):
            raise NstError(f"the anchor of level {level} must have shape ({ch},{h},{w}), got {tuple(anchor.shape)}")
        anchor = anchor.contiguous()
        _chk_dev(anchor, self.device)
        if weights is not None:
            if weights.numel() != h * w or tuple(weights.shape[-2:]) != (h, w):
                raise NstError(f"the weights of level {level} must have shape ({h},{w}), got {tuple(weights.shape)}")
            weights = weights.contiguous()
            _chk_dev(weights, self.device)
        _lib.check(self.ctx, self.lib.nst_level_set_anchor(self.ctx, int(level), _ptr(anchor), _ptr(weights), gamma,
                                                           _stream(self.device)), "nst_level_set_anchor")

    def clear_anchor(self, level: Optional[int] = None) -> None:
        """No temporal term on one level, or (None) on any configured level."""
        for l in (range(self.levels) if level is None else (level,)):
            self.set_anchor(l, None, gamma=0.0)

    def anchor(self, level: int):
        """(gamma, whether a weight plane is set) of a level (nst_level_anchor); gamma = 0: the level has no anchor."""
        g, wt = C.c_float(), C.c_int()
        _lib.check(self.ctx, self.lib.nst_level_anchor(self.ctx, int(level), C.byref(g), C.byref(wt)), "nst_level_anchor")
        return g.value, bool(wt.value)

    def temporal_losses(self) -> torch.Tensor:
        """(levels,) device tensor: the unweighted tmp of the last closure per level (nst_job_temporal_losses); zeros for
        levels without an anchor and levels outside the last level mask."""
        out = torch.empty(self.levels, dtype=torch.float32, device=self.device)
        _lib.check(self.ctx, self.lib.nst_job_temporal_losses(self.ctx, _ptr(out), _stream(self.device)),
                   "nst_job_temporal_losses")
        return out

    # ---- what the per-map terms (MRF, histogram loss, relaxed EMD) share --------------------------------------
    def _level_style(self, level: int, style: torch.Tensor) -> torch.Tensor:
        """The style image a level's per-map term is made from: checked, contiguous."""
        ch = self.channels
        if style.dim() < 3 or style.numel() != ch * style.shape[-2] * style.shape[-1]:
            raise NstError(f"the style image of level {level} must have shape ({ch},hs,ws), got {tuple(style.shape)}")
        style = style.contiguous()
        _chk_dev(style, self.device)
        return style

    def _map_term_losses(self, symbol: str) -> torch.Tensor:
        out = torch.empty((self.levels, 6), dtype=torch.float32, device=self.device)
        _lib.check(self.ctx, getattr(self.lib, symbol)(self.ctx, _ptr(out), _stream(self.device)), symbol)
        return out

    def _clear_levels(self, setter, level: Optional[int]) -> None:
        for l in (range(self.levels) if level is None else (level,)):
            setter(l, None)

    # ---- the MRF style term (nst_level_set_patches; patch_match.py is the driver) ---------------------------
    def set_patches(self, level: int, style: Optional[torch.Tensor], weights=None, stride: int = 1,
                    epsilon: float = _mrf.DEFAULT_EPSILON) -> None:
        """The MRF term of one level (nst_level_set_patches; Li & Wand 2016): the level total gains sum_i w_i mrf_i, mrf_i
        the mean squared distance of the 3x3 patches of map i to their nearest style patch.  style: the level's style image,
        a device float32 (C,hs,ws) tensor (any leading ones; C = 3, or 1 in luminance mode), which is run through the
        network and whose weighted maps are kept; weights: as mrf_modes.normalize_weights takes them.  Data of the job, not
        a setting: configure(), set_taps, set_pooling and set_color drop it.  style None or zero weights clear the level's
        term."""
        setting = None if style is None else _mrf.normalize_mrf(weights, stride, epsilon, None, self.taps[1])
        if setting is None:
            _lib.check(self.ctx, self.lib.nst_level_set_patches(self.ctx, int(level), None, 0, 0, None, 1, _mrf.DEFAULT_EPSILON,
                                                                _stream(self.device)), "nst_level_set_patches")
            return
        w, stride, eps, _ = setting
        style = self._level_style(level, style)
        _lib.check(self.ctx, self.lib.nst_level_set_patches(self.ctx, int(level), _ptr(style), int(style.shape[-2]), int(style.shape[-1]),
                                                            (C.c_float * 6)(*w), stride, eps, _stream(self.device)),
                   "nst_level_set_patches")

    def clear_patches(self, level: Optional[int] = None) -> None:
        """No MRF term on one level, or (None) on any configured level."""
        self._clear_levels(self.set_patches, level)

    def patches_setting(self, level: int):
        """(weights (6,), stride, epsilon) of a level (nst_level_patches), or None when the level has no term."""
        w, st, eps = (C.c_float * 6)(), C.c_int(), C.c_double()
        _lib.check(self.ctx, self.lib.nst_level_patches(self.ctx, int(level), w, C.byref(st), C.byref(eps)), "nst_level_patches")
        ws = tuple(float(v) for v in w)
        return None if all(v == 0.0 for v in ws) else (ws, st.value, eps.value)

    def patch_losses(self) -> torch.Tensor:
        """(levels, 6) device tensor: the unweighted mrf_i of the last closure by map index (nst_job_patch_losses); zeros for
        maps without the term and levels outside the last level mask."""
        return self._map_term_losses("nst_job_patch_losses")

    def patch_matches(self, level: int, map: int) -> torch.Tensor:
        """(h-2, w-2) int32 device tensor: the nearest style patch of every patch of map index `map` of a level, as the last
        closure found it (nst_level_patch_matches)."""
        h, w = self.level_shape(level)
        mh, mw = h >> TAP_SCALE[map], w >> TAP_SCALE[map]
        out = torch.empty((mh - 2, mw - 2), dtype=torch.int32, device=self.device)
        _lib.check(self.ctx, self.lib.nst_level_patch_matches(self.ctx, int(level), int(map), _ptr(out), _stream(self.device)),
                   "nst_level_patch_matches")
        return out

    def patch_match(self, f: torch.Tensor, fs: torch.Tensor, stride: int = 1, epsilon: float = _mrf.DEFAULT_EPSILON):
        """The match alone (nst_patch_match): f (h,w,C) and fs (hs,ws,C) device float32 maps in NHWC, C = 64, 128, 256 or
        512 -> (nn (h-2,w-2) int32, score (h-2,w-2) float32)."""
        stride, eps = _mrf.check_stride(stride), _mrf.check_epsilon(epsilon)
        _chk_dev(f, self.device)
        _chk_dev(fs, self.device)
        if f.dim() != 3 or fs.dim() != 3 or f.shape[2] != fs.shape[2]:
            raise NstError("f and fs must be (h,w,C) and (hs,ws,C) with the same C")
        h, w, c = f.shape
        idx = torch.empty((h - 2, w - 2), dtype=torch.int32, device=self.device)
        score = torch.empty((h - 2, w - 2), dtype=torch.float32, device=self.device)
        _lib.check(self.ctx, self.lib.nst_patch_match(self.ctx, _ptr(f), h, w, c, _ptr(fs), fs.shape[0], fs.shape[1], stride, eps,
                                                      _ptr(idx), _ptr(score), _stream(self.device)), "nst_patch_match")
        return idx, score

    def patch_term(self, f: torch.Tensor, fs: torch.Tensor, idx: torch.Tensor, stride: int = 1, coef: Optional[float] = None,
                   want_grad: bool = True):
        """Value and gradient alone at the given matches (nst_patch_term): mrf (device scalar) and, with want_grad, the
        (h,w,C) gradient under `coef` (None: 2 / (9 C n), the gradient of mrf itself)."""
        stride = _mrf.check_stride(stride)
        _chk_dev(f, self.device)
        _chk_dev(fs, self.device)
        if f.dim() != 3 or fs.dim() != 3 or f.shape[2] != fs.shape[2]:
            raise NstError("f and fs must be (h,w,C) and (hs,ws,C) with the same C")
        h, w, c = f.shape
        if not (idx.is_cuda and idx.dtype == torch.int32 and idx.is_contiguous() and idx.numel() == (h - 2) * (w - 2)):
            raise NstError(f"idx must be a contiguous int32 CUDA tensor of {(h - 2) * (w - 2)} entries")
        if coef is None:
            coef = 2.0 / (9.0 * c * (h - 2) * (w - 2))
        val = torch.empty(1, dtype=torch.float32, device=self.device)
        grad = torch.empty_like(f) if want_grad else None
        _lib.check(self.ctx, self.lib.nst_patch_term(self.ctx, _ptr(f), h, w, c, _ptr(fs), fs.shape[0], fs.shape[1], stride, _ptr(idx),
                                                     float(coef), _ptr(val), _ptr(grad), _stream(self.device)), "nst_patch_term")
        return (val, grad) if want_grad else val

    # ---- the MRF term under semantic maps (nst_level_set_patch_guidance; neural-doodle) ----------------------
    def _semantic_planes(self, planes: torch.Tensor, shape, what: str) -> torch.Tensor:
        if not (isinstance(planes, torch.Tensor) and planes.dtype == torch.float32 and planes.dim() == 3):
            raise ValueError(f"{what}: expected a float32 (R,h,w) device tensor")
        if not 1 <= planes.shape[0] <= _regions.MAX_REGIONS:
            raise ValueError(f"{what}: {planes.shape[0]} regions, 1 .. {_regions.MAX_REGIONS} allowed")
        if shape is not None and tuple(planes.shape[1:]) != tuple(shape):
            raise ValueError(f"{what}: planes of {tuple(planes.shape[1:])}, expected {tuple(shape)}")
        planes = planes.contiguous()
        _chk_dev(planes, self.device)
        return planes

    def set_patch_guidance(self, level: int, content_planes: Optional[torch.Tensor], style_planes: Optional[torch.Tensor],
                           gamma: float = 1.0) -> None:
        """Semantic maps steer the patch search of a level that carries the MRF term (nst_level_set_patch_guidance;
        Champandard 2016): the score of a candidate becomes cos(i,j) + gamma <d_i, e_j>, d and e the normalised nine-tap sums
        of the pooled planes.  content_planes: device float32 (R,h,w) at the level image's size; style_planes: (R,hs,ws) at the
        size of the style image given to set_patches; values in [0,1]; R <= 4.  Call it after set_patches: whatever drops the
        level's term drops its guidance.  None planes or gamma 0 clear the guidance.  ValueError, before the call, for planes
        of another shape or dtype, mismatched R, or a negative or non-finite gamma."""
        g = float(gamma)
        if not np.isfinite(g) or g < 0.0:
            raise ValueError(f"the semantic weight must be finite and >= 0, got {gamma!r}")
        if content_planes is None or style_planes is None or g == 0.0:
            _lib.check(self.ctx, self.lib.nst_level_set_patch_guidance(self.ctx, int(level), 0, None, None, 0.0, _stream(self.device)),
                       "nst_level_set_patch_guidance")
            return
        hs, ws = C.c_int(), C.c_int()
        _lib.check(self.ctx, self.lib.nst_level_patch_guidance(self.ctx, int(level), None, None, C.byref(hs), C.byref(ws)),
                   "nst_level_patch_guidance")
        c = self._semantic_planes(content_planes, self.level_shape(level), "content_planes")
        # (a level without the term has no style size: the call itself refuses it, NST_E_STATE)
        s = self._semantic_planes(style_planes, (hs.value, ws.value) if hs.value > 0 else None, "style_planes")
        if c.shape[0] != s.shape[0]:
            raise ValueError(f"content_planes has {c.shape[0]} regions, style_planes {s.shape[0]}")
        _lib.check(self.ctx, self.lib.nst_level_set_patch_guidance(self.ctx, int(level), int(c.shape[0]), _ptr(c), _ptr(s), g,
                                                                   _stream(self.device)), "nst_level_set_patch_guidance")

    def clear_patch_guidance(self, level: Optional[int] = None) -> None:
        """An unguided search on one level, or (None) on every configured level."""
        for l in (range(self.levels) if level is None else (level,)):
            self.set_patch_guidance(l, None, None)

    def patch_guidance(self, level: int):
        """(R, gamma) of a level (nst_level_patch_guidance), or None when its search is unguided."""
        r, g = C.c_int(), C.c_float()
        _lib.check(self.ctx, self.lib.nst_level_patch_guidance(self.ctx, int(level), C.byref(r), C.byref(g), None, None),
                   "nst_level_patch_guidance")
        return None if r.value == 0 else (r.value, float(g.value))

    def patch_descriptors(self, planes: torch.Tensor, stride: int = 1, epsilon: float = _mrf.DEFAULT_EPSILON) -> torch.Tensor:
        """The semantic descriptors alone (nst_patch_descriptors): planes (R,hm,wm), device float32 at the MAP's resolution
        (regions.pool_chain restates the pooling) -> (count, 4) float32, count the entries of the stride-`stride` geometry:
        stride 1 for the image patches, the style stride for a dictionary."""
        stride, eps = _mrf.check_stride(stride), _mrf.check_epsilon(epsilon)
        planes = self._semantic_planes(planes, None, "planes")
        r, hm, wm = planes.shape
        if hm < 3 or wm < 3:
            raise ValueError(f"planes: a map of {hm}x{wm} has no 3x3 patch")
        count = ((hm - 3) // stride + 1) * ((wm - 3) // stride + 1)
        out = torch.empty((count, 4), dtype=torch.float32, device=self.device)
        _lib.check(self.ctx, self.lib.nst_patch_descriptors(self.ctx, _ptr(planes), r, hm, wm, stride, eps, _ptr(out),
                                                            _stream(self.device)), "nst_patch_descriptors")
        return out

    def patch_match_guided(self, f: torch.Tensor, fs: torch.Tensor, d: torch.Tensor, e: torch.Tensor, gamma: float, stride: int = 1,
                           epsilon: float = _mrf.DEFAULT_EPSILON):
        """The guided match alone (nst_patch_match_guided): patch_match's f and fs, the descriptors d (n,4) of the image
        patches and e (m,4) of the dictionary entries (patch_descriptors) and gamma >= 0 -> (nn (h-2,w-2) int32, T (h-2,w-2)
        float32), T(i,j) = cos(i,j) + gamma <d_i, e_j>."""
        stride, eps = _mrf.check_stride(stride), _mrf.check_epsilon(epsilon)
        g = float(gamma)
        if not np.isfinite(g) or g < 0.0:
            raise ValueError(f"the semantic weight must be finite and >= 0, got {gamma!r}")
        _chk_dev(f, self.device)
        _chk_dev(fs, self.device)
        if f.dim() != 3 or fs.dim() != 3 or f.shape[2] != fs.shape[2]:
            raise NstError("f and fs must be (h,w,C) and (hs,ws,C) with the same C")
        h, w, c = f.shape
        n = (h - 2) * (w - 2)
        m = ((fs.shape[0] - 3) // stride + 1) * ((fs.shape[1] - 3) // stride + 1)
        for t, rows, what in ((d, n, "d"), (e, m, "e")):
            _chk_dev(t, self.device)
            if tuple(t.shape) != (rows, 4):
                raise NstError(f"{what} must be ({rows},4), got {tuple(t.shape)}")
        idx = torch.empty((h - 2, w - 2), dtype=torch.int32, device=self.device)
        score = torch.empty((h - 2, w - 2), dtype=torch.float32, device=self.device)
        _lib.check(self.ctx, self.lib.nst_patch_match_guided(self.ctx, _ptr(f), h, w, c, _ptr(fs), fs.shape[0], fs.shape[1], stride, eps,
                                                             _regions.MAX_REGIONS, _ptr(d), _ptr(e), g, _ptr(idx), _ptr(score),
                                                             _stream(self.device)), "nst_patch_match_guided")
        return idx, score

    # ---- the histogram loss (nst_level_set_histograms; histogram_loss.py is the driver) ----------------------
    def set_histograms(self, level: int, style: Optional[torch.Tensor], weights=None, bins: int = _hist.DEFAULT_BINS) -> None:
        """The histogram loss of one level (nst_level_set_histograms; Risser, Wilmot & Barnes 2017): the level total gains
        sum_i w_i hist_i, hist_i the mean squared distance of map i from its remap onto the style's per-channel histograms.
        style: the level's style image, a device float32 (C,hs,ws) tensor (any leading ones; C = 3, or 1 in luminance mode),
        which is run through the network and of whose weighted maps range and counts are kept; weights: as
        hist_modes.normalize_weights takes them.  Data of the job, not a setting: configure(), set_taps, set_pooling and
        set_color drop it.  style None or zero weights clear the level's term."""
        setting = None if style is None else _hist.normalize_hist(weights, bins, None, self.taps[1])
        if setting is None:
            _lib.check(self.ctx, self.lib.nst_level_set_histograms(self.ctx, int(level), None, 0, 0, None, _hist.DEFAULT_BINS,
                                                                   _stream(self.device)), "nst_level_set_histograms")
            return
        w, bins, _ = setting
        style = self._level_style(level, style)
        _lib.check(self.ctx, self.lib.nst_level_set_histograms(self.ctx, int(level), _ptr(style), int(style.shape[-2]),
                                                               int(style.shape[-1]), (C.c_float * 6)(*w), bins, _stream(self.device)),
                   "nst_level_set_histograms")

    def clear_histograms(self, level: Optional[int] = None) -> None:
        """No histogram loss on one level, or (None) on any configured level."""
        self._clear_levels(self.set_histograms, level)

    def histograms_setting(self, level: int):
        """(weights (6,), bins) of a level (nst_level_histograms), or None when the level has no term."""
        w, b = (C.c_float * 6)(), C.c_int()
        _lib.check(self.ctx, self.lib.nst_level_histograms(self.ctx, int(level), w, C.byref(b)), "nst_level_histograms")
        ws = tuple(float(v) for v in w)
        return None if all(v == 0.0 for v in ws) else (ws, b.value)

    def histogram_losses(self) -> torch.Tensor:
        """(levels, 6) device tensor: the unweighted hist_i of the last closure by map index (nst_job_histogram_losses); zeros
        for maps without the term and levels outside the last level mask."""
        return self._map_term_losses("nst_job_histogram_losses")

    def histogram_tables(self, level: int, map: int):
        """(lo_hi (C,2) float32, counts (C,B) int32, ends (C,B,2) float32) device tensors: the image side of map index `map`
        of a level as the last closure made it (nst_level_histogram_tables)."""
        st = self.histograms_setting(level)
        c, b = TAP_CHANNELS[map], (st[1] if st else _hist.DEFAULT_BINS)
        lo_hi = torch.empty((c, 2), dtype=torch.float32, device=self.device)
        counts = torch.empty((c, b), dtype=torch.int32, device=self.device)
        ends = torch.empty((c, b, 2), dtype=torch.float32, device=self.device)
        _lib.check(self.ctx, self.lib.nst_level_histogram_tables(self.ctx, int(level), int(map), _ptr(lo_hi), _ptr(counts), _ptr(ends),
                                                                 _stream(self.device)), "nst_level_histogram_tables")
        return lo_hi, counts, ends

    def histogram_style(self, level: int, map: int):
        """(lo_hi (C,2) float32, counts (C,B) int32): the style's record of map index `map` of a level
        (nst_level_histogram_style)."""
        st = self.histograms_setting(level)
        c, b = TAP_CHANNELS[map], (st[1] if st else _hist.DEFAULT_BINS)
        lo_hi = torch.empty((c, 2), dtype=torch.float32, device=self.device)
        counts = torch.empty((c, b), dtype=torch.int32, device=self.device)
        _lib.check(self.ctx, self.lib.nst_level_histogram_style(self.ctx, int(level), int(map), _ptr(lo_hi), _ptr(counts),
                                                                _stream(self.device)), "nst_level_histogram_style")
        return lo_hi, counts

    def histogram_counts(self, f: torch.Tensor, bins: int = _hist.DEFAULT_BINS):
        """Range and counts alone (nst_histogram_counts): f (N,C) or (h,w,C) device float32 in NHWC, C = 64, 128, 256 or 512
        -> (lo_hi (C,2) float32, counts (C,B) int32)."""
        bins = _hist.check_bins(bins)
        _chk_dev(f, self.device)
        c = f.shape[-1]
        n = f.numel() // c
        lo_hi = torch.empty((c, 2), dtype=torch.float32, device=self.device)
        counts = torch.empty((c, bins), dtype=torch.int32, device=self.device)
        _lib.check(self.ctx, self.lib.nst_histogram_counts(self.ctx, _ptr(f), n, c, bins, _ptr(lo_hi), _ptr(counts), _stream(self.device)),
                   "nst_histogram_counts")
        return lo_hi, counts

    def histogram_table(self, lo_hi: torch.Tensor, counts: torch.Tensor, n: int, s_lo_hi: torch.Tensor, s_counts: torch.Tensor,
                        ns: int) -> torch.Tensor:
        """The tables alone (nst_histogram_tables): the image's and the style's range and counts (histogram_counts) and their
        pixel counts -> ends (C,B,2) float32."""
        c, bins = counts.shape
        _chk_dev(lo_hi, self.device, (c, 2))
        _chk_dev(s_lo_hi, self.device, (c, 2))
        for t in (counts, s_counts):
            if not (t.is_cuda and t.dtype == torch.int32 and t.is_contiguous() and tuple(t.shape) == (c, bins)):
                raise NstError(f"counts must be contiguous int32 CUDA tensors of shape ({c},{bins})")
        ends = torch.empty((c, bins, 2), dtype=torch.float32, device=self.device)
        _lib.check(self.ctx, self.lib.nst_histogram_tables(self.ctx, _ptr(lo_hi), _ptr(counts), int(n), _ptr(s_lo_hi), _ptr(s_counts),
                                                           int(ns), c, bins, _ptr(ends), _stream(self.device)), "nst_histogram_tables")
        return ends

    def histogram_term(self, f: torch.Tensor, lo_hi: torch.Tensor, ends: torch.Tensor, coef: Optional[float] = None,
                       want_grad: bool = True):
        """Value and gradient alone at the given tables (nst_histogram_term): hist (device scalar) and, with want_grad, the
        gradient in f's shape under `coef` (None: 2 / (C N), the gradient of hist itself)."""
        _chk_dev(f, self.device)
        c = f.shape[-1]
        n = f.numel() // c
        bins = ends.shape[1]
        _chk_dev(lo_hi, self.device, (c, 2))
        _chk_dev(ends, self.device, (c, bins, 2))
        if coef is None:
            coef = 2.0 / (float(c) * n)
        val = torch.empty(1, dtype=torch.float32, device=self.device)
        grad = torch.empty_like(f) if want_grad else None
        _lib.check(self.ctx, self.lib.nst_histogram_term(self.ctx, _ptr(f), n, c, bins, _ptr(lo_hi), _ptr(ends), float(coef), _ptr(val),
                                                         _ptr(grad), _stream(self.device)), "nst_histogram_term")
        return (val, grad) if want_grad else val

    # ---- the relaxed EMD term (nst_level_set_remd; remd_loss.py is the driver) -------------------------------
    def set_remd(self, level: int, style: Optional[torch.Tensor], weights=None, image_strides=1, style_strides=1,
                 epsilon: float = _remd.DEFAULT_EPSILON) -> None:
        """The relaxed EMD term of one level (nst_level_set_remd; Kolkin et al. 2019): the level total gains sum_i w_i remd_i,
        remd_i the larger of the two mean cosine distances of the two-way nearest-neighbour match between the sampled vectors
        of map i and of the style's map i.  style: the level's style image, a device float32 (C,hs,ws) tensor (any leading
        ones; C = 3, or 1 in luminance mode), which is run through the network and whose weighted maps are kept; weights: as
        remd_modes.normalize_weights takes them; image_strides, style_strides: one integer 1..256 or six by map index
        (remd_modes.stride_for chooses one for a sample budget).  Data of the job, not a setting: configure(), set_taps,
        set_pooling and set_color drop it.  style None or zero weights clear the level's term."""
        setting = None if style is None else _remd.normalize_remd(weights, _remd.DEFAULT_SAMPLES, epsilon, None, self.taps[1])
        ones = (C.c_int * 6)(*([1] * 6))
        if setting is None:
            _lib.check(self.ctx, self.lib.nst_level_set_remd(self.ctx, int(level), None, 0, 0, None, ones, ones, _remd.DEFAULT_EPSILON,
                                                             _stream(self.device)), "nst_level_set_remd")
            return
        w, _, eps, _ = setting
        si, ss = _remd.check_strides(image_strides, "image_strides"), _remd.check_strides(style_strides, "style_strides")
        style = self._level_style(level, style)
        _lib.check(self.ctx, self.lib.nst_level_set_remd(self.ctx, int(level), _ptr(style), int(style.shape[-2]), int(style.shape[-1]),
                                                         (C.c_float * 6)(*w), (C.c_int * 6)(*si), (C.c_int * 6)(*ss), eps,
                                                         _stream(self.device)), "nst_level_set_remd")

    def clear_remd(self, level: Optional[int] = None) -> None:
        """No relaxed EMD term on one level, or (None) on any configured level."""
        self._clear_levels(self.set_remd, level)

    def remd_setting(self, level: int):
        """(weights (6,), image strides (6,), style strides (6,), epsilon, (hs, ws) of the style image) of a level
        (nst_level_remd), or None when the level has no term."""
        w, si, ss, eps = (C.c_float * 6)(), (C.c_int * 6)(), (C.c_int * 6)(), C.c_double()
        hs, wd = C.c_int(), C.c_int()
        _lib.check(self.ctx, self.lib.nst_level_remd(self.ctx, int(level), w, si, ss, C.byref(eps), C.byref(hs), C.byref(wd)),
                   "nst_level_remd")
        ws = tuple(float(v) for v in w)
        if all(v == 0.0 for v in ws):
            return None
        return ws, tuple(int(v) for v in si), tuple(int(v) for v in ss), eps.value, (hs.value, wd.value)

    def remd_losses(self) -> torch.Tensor:
        """(levels, 6) device tensor: the unweighted remd_i of the last closure by map index (nst_job_remd_losses); zeros for
        maps without the term and levels outside the last level mask."""
        return self._map_term_losses("nst_job_remd_losses")

    def remd_matches(self, level: int, map: int):
        """(nnA (n,) int32, nnB (m,) int32, side: 0 = A or 1 = B) of map index `map` of a level as the last closure found them
        (nst_level_remd_matches): nnA[i] the style sample of image sample i, nnB[j] the image sample of style sample j."""
        st = self.remd_setting(level)
        if st is None or not st[0][map] > 0.0:
            raise NstError(f"map {map} carries no relaxed EMD term on level {level} (set_remd)")
        h, w = self.level_shape(level)
        n = _remd.samples_of(h >> TAP_SCALE[map], w >> TAP_SCALE[map], st[1][map])
        m = _remd.samples_of(st[4][0] >> TAP_SCALE[map], st[4][1] >> TAP_SCALE[map], st[2][map])
        nna = torch.empty(n, dtype=torch.int32, device=self.device)
        nnb = torch.empty(m, dtype=torch.int32, device=self.device)
        side = torch.empty(1, dtype=torch.int32, device=self.device)
        _lib.check(self.ctx, self.lib.nst_level_remd_matches(self.ctx, int(level), int(map), _ptr(nna), _ptr(nnb), _ptr(side),
                                                             _stream(self.device)), "nst_level_remd_matches")
        return nna, nnb, int(side.item())

    def _remd_maps(self, f: torch.Tensor, fs: torch.Tensor, si, ss, epsilon):
        si, ss, eps = _remd.check_stride(si, "si"), _remd.check_stride(ss, "ss"), _remd.check_epsilon(epsilon)
        _chk_dev(f, self.device)
        _chk_dev(fs, self.device)
        if f.dim() != 3 or fs.dim() != 3 or f.shape[2] != fs.shape[2]:
            raise NstError("f and fs must be (h,w,C) and (hs,ws,C) with the same C")
        n = _remd.samples_of(f.shape[0], f.shape[1], si)
        m = _remd.samples_of(fs.shape[0], fs.shape[1], ss)
        return si, ss, eps, n, m

    def remd_match(self, f: torch.Tensor, fs: torch.Tensor, si: int = 1, ss: int = 1, epsilon: float = _remd.DEFAULT_EPSILON):
        """The match alone (nst_remd_match): f (h,w,C) and fs (hs,ws,C) device float32 maps in NHWC, C = 64, 128, 256 or 512,
        sampled with the strides si and ss -> (nnA (n,) int32, nnB (m,) int32)."""
        si, ss, eps, n, m = self._remd_maps(f, fs, si, ss, epsilon)
        nna = torch.empty(n, dtype=torch.int32, device=self.device)
        nnb = torch.empty(m, dtype=torch.int32, device=self.device)
        _lib.check(self.ctx, self.lib.nst_remd_match(self.ctx, _ptr(f), f.shape[0], f.shape[1], f.shape[2], _ptr(fs), fs.shape[0],
                                                     fs.shape[1], si, ss, eps, _ptr(nna), _ptr(nnb), _stream(self.device)), "nst_remd_match")
        return nna, nnb

    def remd_term(self, f: torch.Tensor, fs: torch.Tensor, nnA: torch.Tensor, nnB: torch.Tensor, si: int = 1, ss: int = 1,
                  epsilon: float = _remd.DEFAULT_EPSILON, side: int = -1, coef: float = 1.0, want_grad: bool = True):
        """Value and gradient alone at the given matches (nst_remd_term): ((remd, rA, rB) device float32, side: 0 = A or 1 = B)
        and, with want_grad, the (h,w,C) gradient of coef remd, zero off the sample grid.  side -1 decides (A when rA >= rB);
        0 or 1 forces that side, and remd is then its r."""
        si, ss, eps, n, m = self._remd_maps(f, fs, si, ss, epsilon)
        if side not in (-1, 0, 1):
            raise ValueError(f"side must be 0 (A), 1 (B) or -1 (decide), not {side!r}")
        for t, rows, what in ((nnA, n, "nnA"), (nnB, m, "nnB")):
            if not (t.is_cuda and t.dtype == torch.int32 and t.is_contiguous() and t.numel() == rows and t.device == self.device):
                raise NstError(f"{what} must be a contiguous int32 CUDA tensor of {rows} entries")
        val = torch.empty(3, dtype=torch.float32, device=self.device)
        sd = torch.empty(1, dtype=torch.int32, device=self.device)
        grad = torch.empty_like(f) if want_grad else None
        _lib.check(self.ctx, self.lib.nst_remd_term(self.ctx, _ptr(f), f.shape[0], f.shape[1], f.shape[2], _ptr(fs), fs.shape[0],
                                                    fs.shape[1], si, ss, eps, _ptr(nnA), _ptr(nnB), int(side), float(coef), _ptr(val),
                                                    _ptr(sd), _ptr(grad), _stream(self.device)), "nst_remd_term")
        return (val, int(sd.item()), grad) if want_grad else (val, int(sd.item()))

    # ---- the self-similarity content term (nst_level_set_selfsim; selfsim_loss.py is the driver) --------------
    def set_selfsim(self, level: int, content: Optional[torch.Tensor], weights=None, strides=1,
                    epsilon: float = _selfsim.DEFAULT_EPSILON) -> None:
        """The self-similarity term of one level (nst_level_set_selfsim; Kolkin et al. 2019): the level total gains
        sum_k w_k selfsim_k, selfsim_k the mean over the sampled positions of the L1 distance between the column-normalised
        cosine-distance matrices of map k and of the content's map k.  content: the level's content image, a device float32
        (C,h,w) tensor of the level's size (any leading ones; C = 3, or 1 in luminance mode), which is run through the network;
        weights: as selfsim_modes.normalize_weights takes them (a number: the job's content map; any map the job uses may
        carry one); strides: one integer 1..256 or six by map index (selfsim_modes.stride_for chooses one for a sample
        budget; at most 4096 samples a map).  Data of the job, not a setting: configure(), set_taps, set_pooling and set_color
        drop it.  content None or zero weights clear the level's term."""
        setting = None if content is None else _selfsim.normalize_selfsim(weights, _selfsim.DEFAULT_SAMPLES, epsilon, None, self.taps[0],
                                                                          self.taps[1])
        if setting is None:
            ones = (C.c_int * 6)(*([1] * 6))
            _lib.check(self.ctx, self.lib.nst_level_set_selfsim(self.ctx, int(level), None, 0, 0, None, ones, _selfsim.DEFAULT_EPSILON,
                                                                _stream(self.device)), "nst_level_set_selfsim")
            return
        w, _, eps, _ = setting
        st = _selfsim.check_strides(strides, "strides")
        ch = self.channels
        if content.dim() < 3 or content.numel() != ch * content.shape[-2] * content.shape[-1]:
            raise NstError(f"the content image of level {level} must have shape ({ch},h,w), got {tuple(content.shape)}")
        content = content.contiguous()
        _chk_dev(content, self.device)
        _lib.check(self.ctx, self.lib.nst_level_set_selfsim(self.ctx, int(level), _ptr(content), int(content.shape[-2]),
                                                            int(content.shape[-1]), (C.c_float * 6)(*w), (C.c_int * 6)(*st), eps,
                                                            _stream(self.device)), "nst_level_set_selfsim")

    def clear_selfsim(self, level: Optional[int] = None) -> None:
        """No self-similarity term on one level, or (None) on any configured level."""
        self._clear_levels(self.set_selfsim, level)

    def selfsim_setting(self, level: int):
        """(weights (6,), strides (6,), epsilon) of a level (nst_level_selfsim), or None when the level has no term."""
        w, st, eps = (C.c_float * 6)(), (C.c_int * 6)(), C.c_double()
        _lib.check(self.ctx, self.lib.nst_level_selfsim(self.ctx, int(level), w, st, C.byref(eps)), "nst_level_selfsim")
        ws = tuple(float(v) for v in w)
        if all(v == 0.0 for v in ws):
            return None
        return ws, tuple(int(v) for v in st), eps.value

    def selfsim_losses(self) -> torch.Tensor:
        """(levels, 6) device tensor: the unweighted selfsim_k of the last closure by map index (nst_job_selfsim_losses); zeros
        for maps without the term and levels outside the last level mask."""
        return self._map_term_losses("nst_job_selfsim_losses")

    def selfsim_decisions(self, level: int, map: int):
        """(D (n,n) float32, s (n,) float64, sg (n,n) int8) of map index `map` of a level as the last closure made them
        (nst_level_selfsim_decisions): D[i, j] the cosine distance with i in the dictionary and j in the column role, s its
        column sums, sg the signs of N - M."""
        st = self.selfsim_setting(level)
        if st is None or not st[0][map] > 0.0:
            raise NstError(f"map {map} carries no self-similarity term on level {level} (set_selfsim)")
        h, w = self.level_shape(level)
        n = _selfsim.samples_of(h >> TAP_SCALE[map], w >> TAP_SCALE[map], st[1][map])
        d = torch.empty((n, n), dtype=torch.float32, device=self.device)
        s = torch.empty(n, dtype=torch.float64, device=self.device)
        sg = torch.empty((n, n), dtype=torch.int8, device=self.device)
        _lib.check(self.ctx, self.lib.nst_level_selfsim_decisions(self.ctx, int(level), int(map), _ptr(d), _ptr(s), _ptr(sg),
                                                                  _stream(self.device)), "nst_level_selfsim_decisions")
        return d, s, sg

    def _selfsim_map(self, f: torch.Tensor, stride, epsilon):
        stride, eps = _selfsim.check_stride(stride, "stride"), _selfsim.check_epsilon(epsilon)
        _chk_dev(f, self.device)
        if f.dim() != 3:
            raise NstError("f must be (h,w,C)")
        n = _selfsim.samples_of(f.shape[0], f.shape[1], stride)
        if n > _selfsim.MAX_SAMPLES:
            raise ValueError(f"stride {stride} leaves {n} samples of a {f.shape[0]}x{f.shape[1]} map: at most {_selfsim.MAX_SAMPLES}")
        return stride, eps, n

    def selfsim_matrix(self, f: torch.Tensor, stride: int = 1, epsilon: float = _selfsim.DEFAULT_EPSILON):
        """The distance matrix alone (nst_selfsim_matrix): f (h,w,C) device float32 map in NHWC, C = 64, 128, 256 or 512,
        sampled with the stride -> (D (n,n) float32, s (n,) float64: the column sums)."""
        stride, eps, n = self._selfsim_map(f, stride, epsilon)
        d = torch.empty((n, n), dtype=torch.float32, device=self.device)
        s = torch.empty(n, dtype=torch.float64, device=self.device)
        _lib.check(self.ctx, self.lib.nst_selfsim_matrix(self.ctx, _ptr(f), f.shape[0], f.shape[1], f.shape[2], stride, eps, _ptr(d),
                                                         _ptr(s), _stream(self.device)), "nst_selfsim_matrix")
        return d, s

    def selfsim_term(self, f: torch.Tensor, fc: torch.Tensor, stride: int = 1, epsilon: float = _selfsim.DEFAULT_EPSILON,
                     coef: float = 1.0, want_grad: bool = True):
        """Value, decisions and gradient alone (nst_selfsim_term): f against the content's map fc, both (h,w,C) ->
        (selfsim device scalar, sg (n,n) int8) and, with want_grad, the (h,w,C) gradient of coef selfsim at those decisions,
        zero off the sample grid."""
        stride, eps, n = self._selfsim_map(f, stride, epsilon)
        _chk_dev(fc, self.device)
        if tuple(fc.shape) != tuple(f.shape):
            raise NstError("f and fc must have the same (h,w,C) shape")
        val = torch.empty(1, dtype=torch.float32, device=self.device)
        sg = torch.empty((n, n), dtype=torch.int8, device=self.device)
        grad = torch.empty_like(f) if want_grad else None
        _lib.check(self.ctx, self.lib.nst_selfsim_term(self.ctx, _ptr(f), _ptr(fc), f.shape[0], f.shape[1], f.shape[2], stride, eps,
                                                       float(coef), _ptr(val), _ptr(sg), _ptr(grad), _stream(self.device)),
                   "nst_selfsim_term")
        return (val, sg, grad) if want_grad else (val, sg)

    # ---- the long-range style term, xcorr (nst_level_set_xcorr; xcorr_loss.py is the driver) -------------------
    def set_xcorr(self, level: int, style: Optional[torch.Tensor], weights=None, shifts=_xcorr.DEFAULT_SHIFTS) -> None:
        """The long-range style term of one level (nst_level_set_xcorr; Berger & Memisevic 2017): the level total gains
        sum_i w_i xcorr_i, xcorr_i the mean over the shifts d of the mean squared difference between G_d = (1/Z_d) sum_p
        F(p + d) F(p)^T of map i and the same statistic of the style's map.  style: the level's style image, a device float32
        (C,hs,ws) tensor (any leading ones; C = 3, or 1 in luminance mode), which is run through the network; weights: as
        xcorr_modes.normalize_weights takes them; shifts: as xcorr_modes.normalize_shifts takes them (an int k: (k, 0) and
        (0, k); a pair (dx, dy) passes through; at most 16 after expansion), each smaller than every weighted map of the level
        and of the style image.  Data of the job, not a setting: configure(), set_taps, set_pooling and set_color drop it.
        style None or zero weights clear the level's term."""
        setting = None if style is None else _xcorr.normalize_xcorr(weights, shifts, None, self.taps[1])
        if setting is None:
            _lib.check(self.ctx, self.lib.nst_level_set_xcorr(self.ctx, int(level), None, 0, 0, None, None, 0, _stream(self.device)),
                       "nst_level_set_xcorr")
            return
        w, sh, _ = setting
        style = self._level_style(level, style)
        _xcorr.level_carries(setting, [self.level_shape(level)], [(int(style.shape[-2]), int(style.shape[-1]))])
        flat = [v for d in sh for v in d]
        _lib.check(self.ctx, self.lib.nst_level_set_xcorr(self.ctx, int(level), _ptr(style), int(style.shape[-2]), int(style.shape[-1]),
                                                          (C.c_float * 6)(*w), (C.c_int * len(flat))(*flat), len(sh),
                                                          _stream(self.device)), "nst_level_set_xcorr")

    def clear_xcorr(self, level: Optional[int] = None) -> None:
        """No xcorr term on one level, or (None) on any configured level."""
        self._clear_levels(self.set_xcorr, level)

    def xcorr_setting(self, level: int):
        """(weights (6,), shifts ((dx, dy), ...), (hs, ws) of the style image) of a level (nst_level_xcorr), or None when the
        level has no term."""
        w, sh, n = (C.c_float * 6)(), (C.c_int * (2 * _xcorr.MAX_SHIFTS))(), C.c_int()
        hs, wd = C.c_int(), C.c_int()
        _lib.check(self.ctx, self.lib.nst_level_xcorr(self.ctx, int(level), w, sh, C.byref(n), C.byref(hs), C.byref(wd)), "nst_level_xcorr")
        ws = tuple(float(v) for v in w)
        if all(v == 0.0 for v in ws):
            return None
        return ws, tuple((int(sh[2 * d]), int(sh[2 * d + 1])) for d in range(n.value)), (hs.value, wd.value)

    def xcorr_losses(self) -> torch.Tensor:
        """(levels, 6) device tensor: the unweighted xcorr_i of the last closure by map index (nst_job_xcorr_losses); zeros for
        maps without the term and levels outside the last level mask."""
        return self._map_term_losses("nst_job_xcorr_losses")

    def xcorr_matrices(self, level: int, map: int) -> torch.Tensor:
        """(|D|, C, C) device float32: the G_d stack of map index `map` of a level as the last closure made it
        (nst_level_xcorr_matrices); zeros before any closure."""
        st = self.xcorr_setting(level)
        if st is None or not st[0][map] > 0.0:
            raise NstError(f"map {map} carries no xcorr term on level {level} (set_xcorr)")
        ch = TAP_CHANNELS[map]
        out = torch.empty((len(st[1]), ch, ch), dtype=torch.float32, device=self.device)
        _lib.check(self.ctx, self.lib.nst_level_xcorr_matrices(self.ctx, int(level), int(map), _ptr(out), _stream(self.device)),
                   "nst_level_xcorr_matrices")
        return out

    def _xcorr_map(self, f: torch.Tensor, shifts):
        _chk_dev(f, self.device)
        if f.dim() != 3:
            raise NstError("f must be (h,w,C)")
        sh = _xcorr.normalize_shifts(shifts)
        _xcorr.check_map(f.shape[0], f.shape[1], sh)
        flat = [v for d in sh for v in d]
        return sh, (C.c_int * len(flat))(*flat)

    def xcorr(self, f: torch.Tensor, shifts=_xcorr.DEFAULT_SHIFTS, want_geometry: bool = False):
        """The statistic alone (nst_xcorr): f (h,w,C) device float32 map in NHWC, C = 64, 128, 256 or 512 -> the (|D|, C, C)
        stack of G_d, d in the order of xcorr_modes.normalize_shifts(shifts); with want_geometry also ((nsplit, pix_per_split),
        ...) per shift: how the device dealt the pairs to its partial sums."""
        sh, arr = self._xcorr_map(f, shifts)
        f = f.contiguous()
        out = torch.empty((len(sh), f.shape[2], f.shape[2]), dtype=torch.float32, device=self.device)
        geo = (C.c_int * (2 * len(sh)))()
        _lib.check(self.ctx, self.lib.nst_xcorr(self.ctx, _ptr(f), f.shape[0], f.shape[1], f.shape[2], arr, len(sh), _ptr(out), geo,
                                                _stream(self.device)), "nst_xcorr")
        if want_geometry:
            return out, tuple((int(geo[2 * d]), int(geo[2 * d + 1])) for d in range(len(sh)))
        return out

    def xcorr_term(self, f: torch.Tensor, gt: torch.Tensor, shifts=_xcorr.DEFAULT_SHIFTS, coef: float = 1.0, want_grad: bool = True):
        """Value and gradient alone (nst_xcorr_term): f (h,w,C) against the targets gt (|D|, C, C) -> the unweighted xcorr as a
        device scalar and, with want_grad, the (h,w,C) gradient of coef xcorr."""
        sh, arr = self._xcorr_map(f, shifts)
        f = f.contiguous()
        _chk_dev(gt, self.device)
        if tuple(gt.shape) != (len(sh), f.shape[2], f.shape[2]):
            raise NstError(f"gt must be ({len(sh)},{f.shape[2]},{f.shape[2]}), got {tuple(gt.shape)}")
        gt = gt.contiguous()
        val = torch.empty(1, dtype=torch.float32, device=self.device)
        grad = torch.empty_like(f) if want_grad else None
        _lib.check(self.ctx, self.lib.nst_xcorr_term(self.ctx, _ptr(f), f.shape[0], f.shape[1], f.shape[2], _ptr(gt), arr, len(sh),
                                                     float(coef), _ptr(val), _ptr(grad), _stream(self.device)), "nst_xcorr_term")
        return (val, grad) if want_grad else val

    def closure(self, x: torch.Tensor, cw: float, sw: float, tvw: float,
                grad: Optional[torch.Tensor] = None, losses: Optional[torch.Tensor] = None):
        """Asynchronous on the current stream. Returns (grad (C,H,W), losses (4*levels+1,)) device tensors (C = 3, or 1
        in luminance mode)."""
        H, W = self.shape
        _chk_dev(x, self.device)
        if x.numel() != self.channels * H * W:
            raise NstError("x has the wrong number of elements")
        if grad is None:
            grad = torch.empty((1, self.channels, H, W), dtype=torch.float32, device=self.device)
        elif grad.numel() != self.channels * H * W:
            raise NstError("grad has the wrong number of elements")
        if losses is None:
            losses = torch.empty(NST_LOSS_ROW * self.levels + 1, dtype=torch.float32, device=self.device)
        _lib.check(self.ctx, self.lib.nst_closure(self.ctx, _ptr(x), cw, sw, tvw, _ptr(grad), _ptr(losses),
                                                  _stream(self.device)), "nst_closure")
        return grad, losses

    def closure_levels(self, x: torch.Tensor, cw: float, sw: float, tvw: float, mask: int,
                       grad: Optional[torch.Tensor] = None, losses: Optional[torch.Tensor] = None):
        """The closure restricted to the levels in `mask` (level sharding); see nst_closure_levels."""
        H, W = self.shape
        _chk_dev(x, self.device)
        if x.numel() != self.channels * H * W:
            raise NstError("x has the wrong number of elements")
        if grad is None:
            grad = torch.empty((1, self.channels, H, W), dtype=torch.float32, device=self.device)
        elif grad.numel() != self.channels * H * W:
            raise NstError("grad has the wrong number of elements")
        if losses is None:
            losses = torch.empty(NST_LOSS_ROW * self.levels + 1, dtype=torch.float32, device=self.device)
        _lib.check(self.ctx, self.lib.nst_closure_levels(self.ctx, _ptr(x), cw, sw, tvw, mask, _ptr(grad),
                                                         _ptr(losses), _stream(self.device)), "nst_closure_levels")
        return grad, losses

    def closure_forward(self, x: torch.Tensor, cw: float, sw: float, tvw: float, mask: int = 0xFFFFFFFF,
                        losses: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The forward half of the closure (nst_closure_forward): the loss row alone, bitwise closure()'s.  NstError
        with code NST_E_UNAVAILABLE outside the batched schedule."""
        _chk_dev(x, self.device)
        if x.numel() != self.channels * self.shape[0] * self.shape[1]:
            raise NstError("x has the wrong number of elements")
        if losses is None:
            losses = torch.empty(NST_LOSS_ROW * self.levels + 1, dtype=torch.float32, device=self.device)
        _lib.check(self.ctx, self.lib.nst_closure_forward(self.ctx, _ptr(x), cw, sw, tvw, mask, _ptr(losses),
                                                          _stream(self.device)), "nst_closure_forward")
        return losses

    def closure_backward(self, x: torch.Tensor, cw: float, sw: float, tvw: float, mask: int = 0xFFFFFFFF,
                         grad: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The backward half of the last closure_forward (nst_closure_backward): the gradient, bitwise closure()'s.  Valid
        only with that call's arguments and while nothing else has used the context since; else NstError (NST_E_STATE)."""
        H, W = self.shape
        _chk_dev(x, self.device)
        if grad is None:
            grad = torch.empty((1, self.channels, H, W), dtype=torch.float32, device=self.device)
        elif grad.numel() != self.channels * H * W:
            raise NstError("grad has the wrong number of elements")
        _lib.check(self.ctx, self.lib.nst_closure_backward(self.ctx, _ptr(x), cw, sw, tvw, mask, _ptr(grad),
                                                           _stream(self.device)), "nst_closure_backward")
        return grad

    # ---- stripe (window) closure: this engine evaluates a horizontal stripe of a larger image (sharding.StripePlan)
    def window_sums_count(self) -> int:
        n = C.c_size_t()
        _lib.check(None, self.lib.nst_window_sums_count(C.byref(n)), "nst_window_sums_count")
        return n.value

    def window_begin(self, xs: torch.Tensor, row0: int, rows: int, H0: int, sums: Optional[torch.Tensor] = None):
        """Forward pass of the stripe image xs (1,3,ext,W0); returns the un-normalised Gram / content / TV sums of the
        owned rows [row0, row0+rows) (see nst_window_begin)."""
        _chk_dev(xs, self.device)
        if sums is None:
            sums = torch.empty(self.window_sums_count(), dtype=torch.float32, device=self.device)
        _lib.check(self.ctx, self.lib.nst_window_begin(self.ctx, _ptr(xs), row0, rows, H0, _ptr(sums), _stream(self.device)),
                   "nst_window_begin")
        return sums

    def window_end(self, xs: torch.Tensor, row0: int, rows: int, H0: int, cw: float, sw: float, tvw: float,
                   sums: torch.Tensor):
        """Backward pass for the loss terms of the owned rows, given the sums of ALL stripes; returns (d loss / d xs,
        level loss row (total, content, style, tv, total)) (see nst_window_end)."""
        _chk_dev(xs, self.device)
        _chk_dev(sums, self.device)
        gxs = torch.empty_like(xs)
        losses = torch.empty(NST_LOSS_ROW + 1, dtype=torch.float32, device=self.device)
        _lib.check(self.ctx, self.lib.nst_window_end(self.ctx, _ptr(xs), row0, rows, H0, cw, sw, tvw, _ptr(sums), _ptr(gxs),
                                                     _ptr(losses), _stream(self.device)), "nst_window_end")
        return gxs, losses

    # ---- the optimisers' update arithmetic alone (unit parity) -------------------------------------------
    def adam_step(self, x: torch.Tensor, g: torch.Tensor, m: torch.Tensor, v: torch.Tensor, k: int, lr: float) -> None:
        """One torch.optim.Adam update in place (nst_adam_step): x, m, v from g at step count k with group lr."""
        for t in (x, g, m, v):
            _chk_dev(t, self.device)
            if t.numel() != x.numel():
                raise NstError("x, g, m, v must have the same number of elements")
        _lib.check(self.ctx, self.lib.nst_adam_step(self.ctx, _ptr(x), _ptr(g), _ptr(m), _ptr(v), x.numel(), k, float(lr),
                                                    _stream(self.device)), "nst_adam_step")

    def lbfgs_direction(self, g: torch.Tensor, ys: Sequence[torch.Tensor], ss: Sequence[torch.Tensor], ro: Sequence[float],
                        h_diag: float, form: int = 0) -> torch.Tensor:
        """d = -H g from the curvature pairs (nst_lbfgs_direction); form 0 = inner products, 1 = sequential recursion."""
        _chk_dev(g, self.device)
        m = len(ys)
        for t in list(ys) + list(ss):
            _chk_dev(t, self.device)
            if t.numel() != g.numel():
                raise NstError("history vectors must have g's size")
        yp = (C.c_void_p * max(m, 1))(*[t.data_ptr() for t in ys])
        sp = (C.c_void_p * max(m, 1))(*[t.data_ptr() for t in ss])
        rp = (C.c_float * max(m, 1))(*[float(r) for r in ro])
        d = torch.empty_like(g)
        _lib.check(self.ctx, self.lib.nst_lbfgs_direction(self.ctx, _ptr(g), yp, sp, rp, m, float(h_diag), g.numel(), form,
                                                          _ptr(d), _stream(self.device)), "nst_lbfgs_direction")
        return d

    def conv_mode(self) -> str:
        """How the 3x3 convolutions are evaluated (nst_options.conv_mode; env NST_CONV by default): 'f16x2' (default: two scaled
        fp16 pieces per fp32 operand, 3 MFMAs per product block, fp32 accumulate), 'bf16x3' (three exact bf16
        pieces, 6 MFMAs) or 'f32' (fp32 MFMA)."""
        return {0: "f32", 1: "bf16x3", 2: "f16x2"}[self.lib.nst_conv_mode(self.ctx)]

    def bytes(self) -> int:
        n = C.c_size_t()
        _lib.check(self.ctx, self.lib.nst_ctx_bytes(self.ctx, C.byref(n)), "nst_ctx_bytes")
        return n.value

    # ---- timing ---------------------------------------------------------------------------------
    def set_timing(self, mode: int) -> None:
        _lib.check(self.ctx, self.lib.nst_set_timing(self.ctx, mode), "nst_set_timing")

    def last_closure_ms(self) -> float:
        ms = C.c_float()
        _lib.check(self.ctx, self.lib.nst_last_closure_ms(self.ctx, C.byref(ms)), "nst_last_closure_ms")
        return ms.value

    def last_closure_class(self, cls: int):
        ms, n, fl = C.c_float(), C.c_int(), C.c_double()
        _lib.check(self.ctx, self.lib.nst_last_closure_class(self.ctx, cls, C.byref(ms), C.byref(n), C.byref(fl)),
                   "nst_last_closure_class")
        return ms.value, n.value, fl.value

    def last_closure_launches(self) -> List[dict]:
        """The timed launches of the last closure (set_timing(2)) in launch order, one dict per launch with the fields of
        nst_launch_info: h2_rows ... h2_bands are the kernel shape the conv_h2 launcher reported (h2_rows = 0: another kernel)."""
        n = C.c_int()
        _lib.check(self.ctx, self.lib.nst_last_closure_launches(self.ctx, None, 0, C.byref(n)), "nst_last_closure_launches")
        buf = (_lib.LaunchInfo * max(n.value, 1))()
        _lib.check(self.ctx, self.lib.nst_last_closure_launches(self.ctx, buf, n.value, C.byref(n)), "nst_last_closure_launches")
        return [{name: getattr(buf[i], name) for name, _ in _lib.LaunchInfo._fields_} for i in range(n.value)]

    def last_closure_schedule(self) -> dict:
        """What the last closure call did with streams and graphs (nst_last_closure_schedule): side_forks, level_streams,
        graph_replay.  Reads host integers of the context: no launch, no wait, no timing mode needed."""
        forks, streams, replay = C.c_int(), C.c_int(), C.c_int()
        _lib.check(self.ctx, self.lib.nst_last_closure_schedule(self.ctx, C.byref(forks), C.byref(streams), C.byref(replay)),
                   "nst_last_closure_schedule")
        return {"side_forks": forks.value, "level_streams": streams.value, "graph_replay": replay.value}

    def timing_totals(self, cls: int, reset: bool = False):
        """(ms, launches, flops) accumulated since the last reset; cls -1 = whole closures."""
        ms, n, fl = C.c_double(), C.c_long(), C.c_double()
        _lib.check(self.ctx, self.lib.nst_timing_totals(self.ctx, cls, C.byref(ms), C.byref(n), C.byref(fl),
                                                        int(reset)), "nst_timing_totals")
        return ms.value, n.value, fl.value

    def timing_mfma_flops(self, cls: int) -> float:
        """Executed matrix-pipe FLOPs of the launches accumulated in timing_totals(cls) (read it BEFORE a resetting call)."""
        fl = C.c_double()
        _lib.check(self.ctx, self.lib.nst_timing_mfma_flops(self.ctx, cls, C.byref(fl)), "nst_timing_mfma_flops")
        return fl.value

    # ---- standalone pieces (unit parity) ----------------------------------------------------------
    def vgg_features(self, x: torch.Tensor) -> List[torch.Tensor]:
        x = x.reshape(3, x.shape[-2], x.shape[-1])
        _chk_dev(x, self.device)
        h, w = x.shape[1], x.shape[2]
        outs = [torch.empty((1, c, h >> s, w >> s), dtype=torch.float32, device=self.device)
                for c, s in zip(TAP_CHANNELS, TAP_SCALE)]
        arr = (C.c_void_p * 6)(*[o.data_ptr() for o in outs])
        _lib.check(self.ctx, self.lib.nst_vgg_features(self.ctx, _ptr(x), h, w, arr, _stream(self.device)),
                   "nst_vgg_features")
        return outs

    def vgg_features_backward(self, x: torch.Tensor, gouts: Sequence[Optional[torch.Tensor]]) -> torch.Tensor:
        x = x.reshape(3, x.shape[-2], x.shape[-1])
        _chk_dev(x, self.device)
        h, w = x.shape[1], x.shape[2]
        for g in gouts:
            if g is not None:
                _chk_dev(g, self.device)
        arr = (C.c_void_p * 6)(*[(g.data_ptr() if g is not None else 0) for g in gouts])
        gx = torch.empty((1, 3, h, w), dtype=torch.float32, device=self.device)
        _lib.check(self.ctx, self.lib.nst_vgg_features_backward(self.ctx, _ptr(x), h, w, arr, _ptr(gx),
                                                                _stream(self.device)), "nst_vgg_features_backward")
        return gx

    LAYER_CHANNELS = (64, 64, 128, 128, 256, 256, 256, 256, 512, 512, 512, 512, 512)
    LAYER_SCALE = (0, 0, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4)

    def vgg_activations(self, x: torch.Tensor) -> List[torch.Tensor]:
        """All 13 post-ReLU conv outputs of a forward pass of x (nst_vgg_activations), each (1,C,h,w)."""
        x = x.reshape(3, x.shape[-2], x.shape[-1])
        _chk_dev(x, self.device)
        h, w = x.shape[1], x.shape[2]
        outs = [torch.empty((1, c, h >> sc, w >> sc), dtype=torch.float32, device=self.device)
                for c, sc in zip(self.LAYER_CHANNELS, self.LAYER_SCALE)]
        arr = (C.c_void_p * 13)(*[o.data_ptr() for o in outs])
        _lib.check(self.ctx, self.lib.nst_vgg_activations(self.ctx, _ptr(x), h, w, arr, _stream(self.device)),
                   "nst_vgg_activations")
        return outs

    def level_activation(self, level: int, layer: int) -> torch.Tensor:
        h, w = self.level_shape(level)
        c, sc = self.LAYER_CHANNELS[layer], self.LAYER_SCALE[layer]
        t = torch.empty((1, c, h >> sc, w >> sc), dtype=torch.float32, device=self.device)
        _lib.check(self.ctx, self.lib.nst_level_activation(self.ctx, level, layer, _ptr(t), _stream(self.device)),
                   "nst_level_activation")
        return t

    def map_stats(self, level: int) -> int:
        """Bit l = the last forward pass of `level` stored conv layer l's full-resolution map, or a level_activation request
        since has written it (nst_job_map_stats)."""
        m = C.c_uint(0)
        _lib.check(self.ctx, self.lib.nst_job_map_stats(self.ctx, level, C.byref(m)), "nst_job_map_stats")
        return int(m.value)

    def level_image(self, level: int) -> torch.Tensor:
        """The (1,C,h,w) image of pyramid level `level` >= 1 that the last closure evaluated (nst_level_image)."""
        h, w = self.level_shape(level)
        t = torch.empty((1, self.channels, h, w), dtype=torch.float32, device=self.device)
        _lib.check(self.ctx, self.lib.nst_level_image(self.ctx, level, _ptr(t), _stream(self.device)), "nst_level_image")
        return t

    def level_activations(self, level: int) -> List[torch.Tensor]:
        """The 13 post-ReLU conv outputs the last closure left in the workspace of `level` (nst_level_activation),
        each (1,C,h,w): what the parity tests derive the device pass's ReLU / pooling decisions from."""
        h, w = self.level_shape(level)
        outs = []
        for l, (c, sc) in enumerate(zip(self.LAYER_CHANNELS, self.LAYER_SCALE)):
            t = torch.empty((1, c, h >> sc, w >> sc), dtype=torch.float32, device=self.device)
            _lib.check(self.ctx, self.lib.nst_level_activation(self.ctx, level, l, _ptr(t), _stream(self.device)),
                       "nst_level_activation")
            outs.append(t)
        return outs

    def gram(self, f: torch.Tensor, normalize: bool = True) -> torch.Tensor:
        _chk_dev(f, self.device)
        b, c, h, w = f.shape
        assert b == 1
        g = torch.empty((1, c, c), dtype=torch.float32, device=self.device)
        _lib.check(self.ctx, self.lib.nst_gram(self.ctx, _ptr(f), c, h, w, int(normalize), _ptr(g),
                                               _stream(self.device)), "nst_gram")
        return g

    def moments(self, f: torch.Tensor, epsilon: float = _mom.DEFAULT_EPSILON):
        """The moment statistic alone (nst_moments): (mu (C,), sigma (C,)) of the (1,C,h,w) map f, sigma = sqrt(var + epsilon),
        the sums in double by the closure's kernels.  C = 64 or a multiple of 128, at most 1024."""
        eps = _mom.check_epsilon(epsilon)
        f = f.contiguous()
        _chk_dev(f, self.device)
        c, h, w = f.shape[-3], f.shape[-2], f.shape[-1]
        mu = torch.empty((c,), dtype=torch.float32, device=self.device)
        sd = torch.empty((c,), dtype=torch.float32, device=self.device)
        _lib.check(self.ctx, self.lib.nst_moments(self.ctx, _ptr(f), c, h, w, eps, _ptr(mu), _ptr(sd), _stream(self.device)), "nst_moments")
        return mu, sd

    def gram_shifted(self, f: torch.Tensor, shift: float = 0.0, center: bool = False, normalize: bool = True):
        """The shifted / centred statistic alone (nst_gram_shifted): (G (1,C,C), o (C,)) of the (1,C,h,w) map f, o = shift
        on every channel or (center) minus the map's channel means."""
        _chk_dev(f, self.device)
        b, c, h, w = f.shape
        assert b == 1
        g = torch.empty((1, c, c), dtype=torch.float32, device=self.device)
        o = torch.empty((c,), dtype=torch.float32, device=self.device)
        _lib.check(self.ctx, self.lib.nst_gram_shifted(self.ctx, _ptr(f), c, h, w, int(normalize), int(bool(center)), float(shift),
                                                       _ptr(g), _ptr(o), _stream(self.device)), "nst_gram_shifted")
        return g, o

    def gram_batch(self, maps, guides=None, targets=None, coefs=None, normalize: bool = True, want_S_bf: bool = False):
        """The closure's batched Gram launch on the caller's maps (nst_gram_batch): one launch for 1 .. 16 (1,C,h,w) maps, C = 64
        or a multiple of 128, under the context's gram_pack.  guides: None, or one (h,w) plane in [0,1] per map (the guided
        form); targets / coefs: None, or per map a (C,C) target or None and its coefficient.  Returns one dict per map: G
        (1,C,C), nsplit and pix_per_split (the launcher's geometry), and with a target S (C,C), mse (the sum of (G - Gt)^2 in
        double), S_absmax and, when asked for, S_bf ((C, C/32, 3, 32) int16 words)."""
        n = len(maps)
        if not 1 <= n <= _lib.NST_GRAM_BATCH_MAX:
            raise NstError(f"a Gram batch takes 1 .. {_lib.NST_GRAM_BATCH_MAX} maps")
        items = (_lib.GramBatchItem * n)()
        outs = []
        for i, f in enumerate(maps):
            _chk_dev(f, self.device)
            b, c, h, w = f.shape
            assert b == 1
            t = targets[i] if targets is not None else None
            g = guides[i] if guides is not None else None
            out = {"G": torch.empty((1, c, c), dtype=torch.float32, device=self.device)}
            if g is not None:
                _chk_dev(g, self.device, (h, w))
            if t is not None:
                _chk_dev(t, self.device, (c, c))
                out["S"] = torch.empty((c, c), dtype=torch.float32, device=self.device)
                if want_S_bf:
                    out["S_bf"] = torch.empty((c, c // 32, 3, 32), dtype=torch.int16, device=self.device)
            items[i].f, items[i].C, items[i].h, items[i].w = f.data_ptr(), c, h, w
            items[i].guide = g.data_ptr() if g is not None else None
            items[i].target = t.data_ptr() if t is not None else None
            items[i].coef = float(coefs[i]) if (coefs is not None and t is not None) else 0.0
            items[i].gram = out["G"].data_ptr()
            items[i].S = out["S"].data_ptr() if "S" in out else None
            items[i].S_bf = out["S_bf"].data_ptr() if "S_bf" in out else None
            outs.append(out)
        _lib.check(self.ctx, self.lib.nst_gram_batch(self.ctx, items, n, int(normalize), _stream(self.device)), "nst_gram_batch")
        for it, out in zip(items, outs):
            out["nsplit"], out["pix_per_split"] = int(it.nsplit), int(it.pix_per_split)
            if "S" in out:
                out["mse"], out["S_absmax"] = float(it.mse), float(it.S_absmax)
        return outs

    def guided_gram_backward(self, f: torch.Tensor, planes: torch.Tensor, s_mats: torch.Tensor, addend: Optional[torch.Tensor] = None,
                             relu_bits: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None, want_absmax: bool = False):
        """The guided Gram backward launch on its own (nst_guided_gram_backward): out (N,C) = addend + sum_r t_r^2 . f . S_r for
        f (N,C), planes (R,N), s_mats (R,C,C), all float32 on the device; relu_bits (N, C/32) int32 words zero the outputs
        whose bit is clear; `out` may be `addend` itself.  Returns out, or (out, max |out| as a device scalar)."""
        n, c = f.shape
        r = planes.shape[0]
        if tuple(planes.shape) != (r, n) or tuple(s_mats.shape) != (r, c, c):
            raise NstError("planes must be (R,N) and s_mats (R,C,C)")
        if out is None:
            out = torch.empty((n, c), dtype=torch.float32, device=self.device)
        slots = torch.empty(64, dtype=torch.int32, device=self.device) if want_absmax else None
        for t in (f, planes, s_mats, addend, out):
            if t is not None:
                _chk_dev(t, self.device)
        if relu_bits is not None and not (relu_bits.is_cuda and relu_bits.dtype == torch.int32 and relu_bits.is_contiguous()
                                          and tuple(relu_bits.shape) == (n, c // 32)):
            raise NstError(f"relu_bits must be a contiguous int32 CUDA tensor of shape ({n},{c // 32})")
        if (addend is not None and addend.shape != f.shape) or out.shape != f.shape:
            raise NstError("addend and out must have the shape of f")
        _lib.check(self.ctx, self.lib.nst_guided_gram_backward(self.ctx, _ptr(f), n, c, r, _ptr(planes), _ptr(s_mats), _ptr(addend),
                                                               _ptr(relu_bits), _ptr(out), _ptr(slots), _stream(self.device)),
                   "nst_guided_gram_backward")
        return (out, slots.view(torch.float32).max()) if want_absmax else out

    def total_variation(self, y: torch.Tensor, want_grad: bool = False):
        _chk_dev(y, self.device)
        b, c, h, w = y.shape
        val = torch.empty(1, dtype=torch.float32, device=self.device)
        grad = torch.empty_like(y) if want_grad else None
        _lib.check(self.ctx, self.lib.nst_total_variation(self.ctx, _ptr(y), b * c, h, w, _ptr(val), _ptr(grad),
                                                          _stream(self.device)), "nst_total_variation")
        return (val, grad) if want_grad else val

    def laplacian_loss(self, y: torch.Tensor, content: torch.Tensor, p: int, want_grad: bool = False):
        """One entry of the Laplacian loss on its own (nst_laplacian_loss): lap of the (1,C,h,w) image y against content
        under pool size p, C = 3 or 1 (a luminance plane); with want_grad also d lap / dy."""
        _chk_dev(y, self.device)
        _chk_dev(content, self.device, y.shape)
        b, c, h, w = y.shape
        val = torch.empty(1, dtype=torch.float32, device=self.device)
        grad = torch.empty_like(y) if want_grad else None
        _lib.check(self.ctx, self.lib.nst_laplacian_loss(self.ctx, _ptr(y), _ptr(content), b * c, h, w, int(p), _ptr(val),
                                                         _ptr(grad), _stream(self.device)), "nst_laplacian_loss")
        return (val, grad) if want_grad else val

    def matting_loss(self, y: torch.Tensor, guide: torch.Tensor, epsilon: float = _mat.DEFAULT_EPSILON, want_grad: bool = False):
        """The matting term on its own (nst_matting_loss): mat of the prepared (1,C,h,w) image y under the guide I (same
        shape, in [0,1] for ordinary input), C = 3 or 1 (a luminance plane under a one-plane guide); with want_grad also
        d mat / dy."""
        eps = _mat.normalize_matting(1.0, epsilon)[1]
        _chk_dev(y, self.device)
        _chk_dev(guide, self.device, y.shape)
        b, c, h, w = y.shape
        val = torch.empty(1, dtype=torch.float32, device=self.device)
        grad = torch.empty_like(y) if want_grad else None
        _lib.check(self.ctx, self.lib.nst_matting_loss(self.ctx, _ptr(y), _ptr(guide), b * c, h, w, eps, _ptr(val),
                                                       _ptr(grad), _stream(self.device)), "nst_matting_loss")
        return (val, grad) if want_grad else val

    def anchor_loss(self, y: torch.Tensor, anchor: torch.Tensor, weights: Optional[torch.Tensor] = None, want_grad: bool = False):
        """The temporal term on its own (nst_anchor_loss): tmp of the (1,C,h,w) image y against the anchor (same shape) under
        the (h,w) weight plane (None: ones), C = 3 or 1; with want_grad also d tmp / dy."""
        _chk_dev(y, self.device)
        _chk_dev(anchor, self.device, y.shape)
        b, c, h, w = y.shape
        if weights is not None:
            _chk_dev(weights, self.device, (h, w))
        val = torch.empty(1, dtype=torch.float32, device=self.device)
        grad = torch.empty_like(y) if want_grad else None
        _lib.check(self.ctx, self.lib.nst_anchor_loss(self.ctx, _ptr(y), _ptr(anchor), _ptr(weights), b * c, h, w, _ptr(val),
                                                      _ptr(grad), _stream(self.device)), "nst_anchor_loss")
        return (val, grad) if want_grad else val

    def anchor_geometry(self) -> Tuple[int, int]:
        """(blocks of the temporal term's value pass, elements a block covers per pass of its loop) (nst_anchor_geometry)."""
        nb, ne = C.c_int(), C.c_int()
        _lib.check(self.ctx, self.lib.nst_anchor_geometry(C.byref(nb), C.byref(ne)), "nst_anchor_geometry")
        return nb.value, ne.value

    def warp_bilinear(self, src: torch.Tensor, flow: torch.Tensor):
        """(out, valid): the (C,h,w) planes src sampled bilinearly at p + flow(p), flow (2,h,w) = (dx, dy) in pixels, and the
        (h,w) plane that is 1 where the four taps lie inside the image (nst_warp_bilinear)."""
        _chk_dev(src, self.device)
        h, w = src.shape[-2:]
        _chk_dev(flow, self.device, (2, h, w))
        out = torch.empty_like(src)
        valid = torch.empty((h, w), dtype=torch.float32, device=self.device)
        _lib.check(self.ctx, self.lib.nst_warp_bilinear(self.ctx, _ptr(src), _ptr(flow), src.numel() // (h * w), h, w, _ptr(out),
                                                        _ptr(valid), _stream(self.device)), "nst_warp_bilinear")
        return out, valid

    def flow_weights(self, fwd: torch.Tensor, bwd: torch.Tensor) -> torch.Tensor:
        """The (h,w) reliability plane of a forward / backward flow pair, (2,h,w) each (nst_flow_weights): 0 at
        disocclusions, motion boundaries and where the backward flow leaves the image, 1 elsewhere."""
        _chk_dev(bwd, self.device)
        _, h, w = bwd.shape
        _chk_dev(bwd, self.device, (2, h, w))
        _chk_dev(fwd, self.device, (2, h, w))
        out = torch.empty((h, w), dtype=torch.float32, device=self.device)
        _lib.check(self.ctx, self.lib.nst_flow_weights(self.ctx, _ptr(fwd), _ptr(bwd), h, w, _ptr(out), _stream(self.device)),
                   "nst_flow_weights")
        return out

    def anchor_fold(self, sources, weights, want_parts: bool = False):
        """(anchor, weight): the one (C,h,w) anchor and (h,w) weight plane that stand for the J = 1 .. 8 `sources` ((C,h,w)
        each, C = 3 or 1: earlier results warped to this frame, ascending in frame offset) under their (h,w) reliability
        planes `weights` (nst_anchor_fold): per pixel a source counts only where no nearer one is reliable.  With want_parts
        also the (J,h,w) planes l_j each source counts with."""
        sources, weights = list(sources), list(weights)
        n = len(sources)
        if not 1 <= n <= _lib.NST_MAX_ANCHOR_SOURCES or len(weights) != n:
            raise ValueError(f"anchor_fold: 1 .. {_lib.NST_MAX_ANCHOR_SOURCES} sources and as many weight planes, got {n} and {len(weights)}")
        _chk_dev(sources[0], self.device)
        if sources[0].dim() != 3:
            raise NstError(f"expected (C,h,w) sources, got {tuple(sources[0].shape)}")
        c, h, w = sources[0].shape
        for s, p in zip(sources, weights):
            _chk_dev(s, self.device, (c, h, w))
            _chk_dev(p, self.device, (h, w))
        anchor = torch.empty_like(sources[0])
        weight = torch.empty((h, w), dtype=torch.float32, device=self.device)
        parts = torch.empty((n, h, w), dtype=torch.float32, device=self.device) if want_parts else None
        src = (C.c_void_p * n)(*[s.data_ptr() for s in sources])
        wts = (C.c_void_p * n)(*[p.data_ptr() for p in weights])
        _lib.check(self.ctx, self.lib.nst_anchor_fold(self.ctx, n, src, wts, c, h, w, _ptr(anchor), _ptr(weight), _ptr(parts),
                                                      _stream(self.device)), "nst_anchor_fold")
        return (anchor, weight, parts) if want_parts else (anchor, weight)

    # ---- the flow estimator (nst_flow_estimate in include/nst_hip.h has the definitions); every buffer is torch's
    def flow_estimate(self, from_plane: torch.Tensor, to_plane: torch.Tensor, params=None) -> torch.Tensor:
        """The (2,h,w) flow w = (u, v) with from(p) ~ to(p + w(p)) of two (h,w) planes on the 0 ... 255 scale of luminance()
        (nst_flow_estimate): multi-scale Horn-Schunck with warping.  `params`: a flow_modes.FlowParams (None: the defaults) -
        or a flow_modes.TVL1Params: TV-L1 on the same pyramid (nst_flow_tvl1_estimate), sharp at motion boundaries."""
        tvl1 = isinstance(params, _flow.TVL1Params)
        p = _flow.normalize_tvl1(params) if tvl1 else _flow.normalize_flow(params)
        _chk_dev(from_plane, self.device)
        h, w = from_plane.shape
        _chk_dev(to_plane, self.device, (h, w))
        floats, _ = (flow_tvl1_workspace if tvl1 else flow_workspace)(h, w, p.scales)
        work = torch.empty(floats, dtype=torch.float32, device=self.device)
        out = torch.empty((2, h, w), dtype=torch.float32, device=self.device)
        if tvl1:
            _lib.check(self.ctx, self.lib.nst_flow_tvl1_estimate(self.ctx, _ptr(from_plane), _ptr(to_plane), h, w, p.lambda_, p.theta,
                                                                 p.tau, p.scales, p.warps, p.iterations, _ptr(out), _ptr(work), floats,
                                                                 _stream(self.device)), "nst_flow_tvl1_estimate")
            return out
        _lib.check(self.ctx, self.lib.nst_flow_estimate(self.ctx, _ptr(from_plane), _ptr(to_plane), h, w, p.alpha, p.scales, p.warps,
                                                        p.iterations, _ptr(out), _ptr(work), floats, _stream(self.device)),
                   "nst_flow_estimate")
        return out

    def flow_reduce(self, plane: torch.Tensor) -> torch.Tensor:
        """One pyramid step of an (h,w) plane: ((h+1)//2, (w+1)//2) (nst_flow_reduce)."""
        _chk_dev(plane, self.device)
        h, w = plane.shape
        out = torch.empty(((h + 1) // 2, (w + 1) // 2), dtype=torch.float32, device=self.device)
        _lib.check(self.ctx, self.lib.nst_flow_reduce(self.ctx, _ptr(plane), h, w, _ptr(out), _stream(self.device)), "nst_flow_reduce")
        return out

    def flow_prolong(self, coarse: torch.Tensor, h: int, w: int) -> torch.Tensor:
        """A (2,(h+1)//2,(w+1)//2) flow on the next finer grid, (2,h,w), its displacements doubled (nst_flow_prolong)."""
        h, w = int(h), int(w)
        _chk_dev(coarse, self.device, (2, (h + 1) // 2, (w + 1) // 2))
        out = torch.empty((2, h, w), dtype=torch.float32, device=self.device)
        _lib.check(self.ctx, self.lib.nst_flow_prolong(self.ctx, _ptr(coarse), h, w, _ptr(out), _stream(self.device)), "nst_flow_prolong")
        return out

    def flow_linearize(self, from_plane: torch.Tensor, to_plane: torch.Tensor, flow: torch.Tensor):
        """(Ix, Iy, rho), (h,w) each: the linearisation of the pair at the (2,h,w) flow (nst_flow_linearize)."""
        _chk_dev(from_plane, self.device)
        h, w = from_plane.shape
        _chk_dev(to_plane, self.device, (h, w))
        _chk_dev(flow, self.device, (2, h, w))
        ix, iy, rho = (torch.empty((h, w), dtype=torch.float32, device=self.device) for _ in range(3))
        _lib.check(self.ctx, self.lib.nst_flow_linearize(self.ctx, _ptr(from_plane), _ptr(to_plane), _ptr(flow), h, w, _ptr(ix), _ptr(iy),
                                                         _ptr(rho), _stream(self.device)), "nst_flow_linearize")
        return ix, iy, rho

    def flow_sweeps(self, ix: torch.Tensor, iy: torch.Tensor, rho: torch.Tensor, flow: torch.Tensor, alpha: float, n: int) -> torch.Tensor:
        """The (2,h,w) flow after n Jacobi sweeps from `flow` under the linearisation (ix, iy, rho) (nst_flow_sweeps)."""
        _chk_dev(flow, self.device)
        _, h, w = flow.shape
        _chk_dev(flow, self.device, (2, h, w))
        for t in (ix, iy, rho):
            _chk_dev(t, self.device, (h, w))
        out = torch.empty_like(flow)
        scratch = torch.empty_like(flow) if int(n) > 1 else None
        _lib.check(self.ctx, self.lib.nst_flow_sweeps(self.ctx, _ptr(ix), _ptr(iy), _ptr(rho), _ptr(flow), h, w, float(alpha), int(n),
                                                      _ptr(out), _ptr(scratch), _stream(self.device)), "nst_flow_sweeps")
        return out

    def flow_tvl1_iterations(self, ix: torch.Tensor, iy: torch.Tensor, rho: torch.Tensor, flow: torch.Tensor, dual: torch.Tensor,
                             lambda_: float, theta: float, tau: float, n: int):
        """(flow (2,h,w), duals (4,h,w)) after n TV-L1 iterations from `flow` and `dual` (p11, p12, p21, p22) under the
        linearisation (ix, iy, rho) (nst_flow_tvl1_iterations)."""
        _chk_dev(flow, self.device)
        _, h, w = flow.shape
        _chk_dev(flow, self.device, (2, h, w))
        _chk_dev(dual, self.device, (4, h, w))
        for t in (ix, iy, rho):
            _chk_dev(t, self.device, (h, w))
        out, dual_out = torch.empty_like(flow), torch.empty_like(dual)
        scratch = torch.empty((6, h, w), dtype=torch.float32, device=self.device) if int(n) > 1 else None
        _lib.check(self.ctx, self.lib.nst_flow_tvl1_iterations(self.ctx, _ptr(ix), _ptr(iy), _ptr(rho), _ptr(flow), _ptr(dual), h, w,
                                                               float(lambda_), float(theta), float(tau), int(n), _ptr(out),
                                                               _ptr(dual_out), _ptr(scratch), _stream(self.device)),
                   "nst_flow_tvl1_iterations")
        return out, dual_out

    def bicubic_half(self, x: torch.Tensor) -> torch.Tensor:
        _chk_dev(x, self.device)
        b, c, h, w = x.shape
        y = torch.empty((b, c, h // 2, w // 2), dtype=torch.float32, device=self.device)
        _lib.check(self.ctx, self.lib.nst_bicubic_half(self.ctx, _ptr(x), b * c, h, w, _ptr(y), _stream(self.device)),
                   "nst_bicubic_half")
        return y

    def bicubic_half_backward(self, gy: torch.Tensor, h: int, w: int) -> torch.Tensor:
        _chk_dev(gy, self.device)
        b, c = gy.shape[0], gy.shape[1]
        gx = torch.empty((b, c, h, w), dtype=torch.float32, device=self.device)
        _lib.check(self.ctx, self.lib.nst_bicubic_half_backward(self.ctx, _ptr(gy), b * c, h, w, _ptr(gx),
                                                                _stream(self.device)), "nst_bicubic_half_backward")
        return gx

    def prepare_img(self, hwc: torch.Tensor) -> torch.Tensor:
        _chk_dev(hwc, self.device)
        h, w, _ = hwc.shape
        out = torch.empty((1, 3, h, w), dtype=torch.float32, device=self.device)
        _lib.check(self.ctx, self.lib.nst_prepare_img(self.ctx, _ptr(hwc), h, w, _ptr(out), _stream(self.device)),
                   "nst_prepare_img")
        return out

    def unprepare_img(self, chw: torch.Tensor) -> torch.Tensor:
        _chk_dev(chw, self.device)
        h, w = chw.shape[-2], chw.shape[-1]
        out = torch.empty((h, w, 3), dtype=torch.float32, device=self.device)
        _lib.check(self.ctx, self.lib.nst_unprepare_img(self.ctx, _ptr(chw), h, w, _ptr(out), _stream(self.device)),
                   "nst_unprepare_img")
        return out


    # ---- job set-up on the device -------------------------------------
    def resize(self, img: torch.Tensor, nh: int, nw: int) -> torch.Tensor:
        """cv2.INTER_CUBIC resize of an (h,w,c) float32 device image."""
        _chk_dev(img, self.device)
        h, w, c = img.shape
        out = torch.empty((nh, nw, c), dtype=torch.float32, device=self.device)
        _lib.check(self.ctx, self.lib.nst_resize_bicubic(self.ctx, _ptr(img), h, w, c, _ptr(out), nh, nw,
                                                         _stream(self.device)), "nst_resize_bicubic")
        return out

    def gather_rows(self, src: torch.Tensor, perm: torch.Tensor) -> torch.Tensor:
        _chk_dev(src, self.device)
        assert perm.dtype == torch.int64 and perm.is_cuda and perm.is_contiguous()
        out = torch.empty_like(src)
        _lib.check(self.ctx, self.lib.nst_gather_rows(self.ctx, _ptr(src), _ptr(perm), perm.numel(), src.shape[-1],
                                                      _ptr(out), _stream(self.device)), "nst_gather_rows")
        return out

    def gaussian_mask_accumulate(self, acc: torch.Tensor, src: Optional[torch.Tensor], central: float,
                                 peripheral: float, dispersion: float) -> None:
        _chk_dev(acc, self.device)
        h, w, c = acc.shape
        if src is not None:
            _chk_dev(src, self.device, acc.shape)
        _lib.check(self.ctx, self.lib.nst_gaussian_mask_accumulate(self.ctx, _ptr(acc), _ptr(src), h, w, c, central,
                                                                   peripheral, dispersion, _stream(self.device)),
                   "nst_gaussian_mask_accumulate")

    def noise_blend(self, content: torch.Tensor, noise: torch.Tensor, noise_factor: float) -> torch.Tensor:
        _chk_dev(content, self.device)
        _chk_dev(noise, self.device, content.shape)
        h, w, c = content.shape
        out = torch.empty_like(content)
        _lib.check(self.ctx, self.lib.nst_noise_blend(self.ctx, _ptr(content), _ptr(noise), h, w, c, noise_factor,
                                                      _ptr(out), _stream(self.device)), "nst_noise_blend")
        return out

    def scale(self, src: torch.Tensor, alpha: float) -> torch.Tensor:
        _chk_dev(src, self.device)
        out = torch.empty_like(src)
        _lib.check(self.ctx, self.lib.nst_scale(self.ctx, _ptr(src), alpha, src.numel(), _ptr(out),
                                                _stream(self.device)), "nst_scale")
        return out

    # ---- colour preservation set-up (Gatys et al. 2016; host_image.py restates these in fp64) ----
    def color_stats(self, hwc: torch.Tensor):
        """(mean (3,), population covariance (3,3)) float64 numpy of an (h,w,3) device image (nst_color_stats; synchronous)."""
        _chk_dev(hwc, self.device)
        h, w, c = hwc.shape
        if c != 3:
            raise NstError("expected an (h,w,3) image")
        mean, cov = np.zeros(3), np.zeros(9)
        _lib.check(self.ctx, self.lib.nst_color_stats(self.ctx, _ptr(hwc), h, w, mean.ctypes.data_as(C.POINTER(C.c_double)),
                                                      cov.ctypes.data_as(C.POINTER(C.c_double)), _stream(self.device)),
                   "nst_color_stats")
        return mean, cov.reshape(3, 3)

    def color_transfer_matrix(self, stats_c, stats_s):
        """(A (3,3), b (3,)) float64 of nst_color_transfer_matrix: A p + b carries the style statistics to the content's."""
        dp = C.POINTER(C.c_double)
        args = [np.ascontiguousarray(a, dtype=np.float64) for a in (stats_c[0], stats_c[1], stats_s[0], stats_s[1])]
        A, b = np.zeros(9), np.zeros(3)
        _lib.check(None, self.lib.nst_color_transfer_matrix(*[a.ctypes.data_as(dp) for a in args], A.ctypes.data_as(dp),
                                                            b.ctypes.data_as(dp)), "nst_color_transfer_matrix")
        return A.reshape(3, 3), b

    def color_affine(self, hwc: torch.Tensor, A, b) -> torch.Tensor:
        """A p + b per pixel of an (h,w,3) device image (nst_color_affine)."""
        _chk_dev(hwc, self.device)
        h, w, _ = hwc.shape
        dp = C.POINTER(C.c_double)
        A = np.ascontiguousarray(A, dtype=np.float64).reshape(9)
        b = np.ascontiguousarray(b, dtype=np.float64).reshape(3)
        out = torch.empty_like(hwc)
        _lib.check(self.ctx, self.lib.nst_color_affine(self.ctx, _ptr(hwc), h, w, A.ctypes.data_as(dp), b.ctypes.data_as(dp),
                                                       _ptr(out), _stream(self.device)), "nst_color_affine")
        return out

    def luminance(self, hwc: torch.Tensor, alpha: float = 1.0, beta: float = 0.0) -> torch.Tensor:
        """(1,1,h,w) 255 (alpha Y + beta) of an (h,w,3) device image (nst_luminance)."""
        _chk_dev(hwc, self.device)
        h, w, _ = hwc.shape
        out = torch.empty((1, 1, h, w), dtype=torch.float32, device=self.device)
        _lib.check(self.ctx, self.lib.nst_luminance(self.ctx, _ptr(hwc), h, w, float(alpha), float(beta), _ptr(out),
                                                    _stream(self.device)), "nst_luminance")
        return out

    def luminance_recombine(self, u: torch.Tensor, content: torch.Tensor) -> torch.Tensor:
        """(h,w,3) YIQ^-1 (u / 255, I(content), Q(content)) (nst_luminance_recombine)."""
        _chk_dev(u, self.device)
        _chk_dev(content, self.device)
        h, w, _ = content.shape
        if u.numel() != h * w:
            raise NstError("u and content differ in size")
        out = torch.empty((h, w, 3), dtype=torch.float32, device=self.device)
        _lib.check(self.ctx, self.lib.nst_luminance_recombine(self.ctx, _ptr(u), _ptr(content), h, w, _ptr(out),
                                                              _stream(self.device)), "nst_luminance_recombine")
        return out


class PixelOptimizer:
    """nst_opt: torch.optim.Adam / LBFGS as the reference constructs them, driving the closure."""

    def __init__(self, engine: StyleEngine, name: str, lr_start: float = 10.0, lbfgs_max_eval: int = 1):
        if name == "adam":
            kind = _lib.NST_OPT_ADAM
        elif name == "lbfgs":
            kind = _lib.NST_OPT_LBFGS
        else:
            raise RuntimeError("Unknown optimizer")   # neural_style_transfer.py:137-138
        self.engine = engine
        self.name = name
        h = C.c_void_p()
        _lib.check(engine.ctx, engine.lib.nst_opt_create(engine.ctx, kind, lr_start, lbfgs_max_eval, C.byref(h)),
                   "nst_opt_create")
        self.h = h
        self.channels = engine.channels
        self.row = NST_LOSS_ROW * engine.levels + 1
        self.cap = 32 if name == "lbfgs" else 1
        self._rows = np.zeros((self.cap, self.row), dtype=np.float32)

    def shard_levels_comm(self, comm: "Communicator") -> None:
        """Level sharding with the collective behind the C ABI (nst_opt_shard_levels_comm): one ncclAllReduce of the packed
        gradient + loss row per closure on the job's stream, no Python in the loop."""
        from . import sharding
        e = self.engine
        self._comm = comm
        _lib.check(e.ctx, e.lib.nst_opt_shard_levels_comm(self.h, sharding.level_mask(e.levels, comm.rank, comm.world),
                                                          comm.h), "nst_opt_shard_levels_comm")

    def history(self):
        """(curvature pairs held, optimiser iteration count)."""
        p, n = C.c_int(), C.c_int()
        _lib.check(self.engine.ctx, self.engine.lib.nst_opt_history(self.h, C.byref(p), C.byref(n)), "nst_opt_history")
        return p.value, n.value

    def set_closure_reuse(self, enabled: bool) -> None:
        """L-BFGS: serve a step's first closure from the previous step when x is bitwise the image that step left
        (nst_opt_set_closure_reuse; default on, env NST_CLOSURE_REUSE=0 off).  Results are the same either way."""
        _lib.check(self.engine.ctx, self.engine.lib.nst_opt_set_closure_reuse(self.h, int(bool(enabled))),
                   "nst_opt_set_closure_reuse")

    def closure_stats(self):
        """(closures evaluated, closures served) so far."""
        ev, sv = C.c_long(), C.c_long()
        _lib.check(self.engine.ctx, self.engine.lib.nst_opt_closure_stats(self.h, C.byref(ev), C.byref(sv)),
                   "nst_opt_closure_stats")
        return ev.value, sv.value

    def set_lazy_backward(self, enabled: bool) -> None:
        """L-BFGS: evaluate the last trial point a line-search budget allows by its forward half and run the backward
        half only when the point is taken (nst_opt_set_lazy_backward; default on, env NST_LAZY_BACKWARD=0 off).  Results
        are the same either way."""
        _lib.check(self.engine.ctx, self.engine.lib.nst_opt_set_lazy_backward(self.h, int(bool(enabled))),
                   "nst_opt_set_lazy_backward")

    def backward_stats(self):
        """(closures evaluated by their forward half only, those of them whose backward half never ran) so far."""
        fo, sk = C.c_long(), C.c_long()
        _lib.check(self.engine.ctx, self.engine.lib.nst_opt_backward_stats(self.h, C.byref(fo), C.byref(sk)),
                   "nst_opt_backward_stats")
        return fo.value, sk.value

    def shard_levels(self, rank: int, world: int, dist_mod=None, group=None) -> None:
        """Level sharding (BASELINE config 4): this rank evaluates only its levels; after every closure
        the partial gradient and loss rows are all-reduced (RCCL) before the driver reads them."""
        from . import sharding
        e = self.engine
        H, W = e.shape
        self._g = torch.zeros((1, self.channels, H, W), dtype=torch.float32, device=e.device)
        self._l = torch.zeros(self.row, dtype=torch.float32, device=e.device)

        def hook(_user):
            sharding.allreduce_closure(self._g, self._l, dist_mod, group)

        self._hook = _lib.REDUCE_HOOK(hook)          # keep the callback object alive
        _lib.check(e.ctx, e.lib.nst_opt_shard_levels(self.h, sharding.level_mask(e.levels, rank, world),
                                                     _ptr(self._g), _ptr(self._l), self._hook, None),
                   "nst_opt_shard_levels")

    def shard_stripes(self, rank: int, world: int, weights, content_t, style_t,
                      dist_mod=None, group=None, comm: "Communicator" = None, blend=None) -> None:
        """Spatial sharding of the large levels (SURVEY 8(e) partition B, halo recompute) on top of level sharding of the
        rest: every rank evaluates a horizontal stripe (its rows + a 96-row halo, a single-level engine of its own) of
        every STRIPED level and its share of the other levels.  content_t / style_t: the prepared (1,3,h,w) content and
        (1,3,hs,ws) style images of the striped levels, level 0 first - a tensor (level 0 only, 75 % of the work) or a
        list (levels 0, 1, ...: with level 1 striped as well 94 % of the work is cut evenly).  Per closure: ONE
        all-reduce of the Gram / content / TV sums of all striped levels between the stripes' forward and backward passes,
        one of the pixel gradient and the loss rows at the end.  A striped level l >= 1 works on the rows of
        x_l = D^l x (the whole down-sampled image is formed on every rank: HBM-bound, 1/4 of the pixels) and hands its
        partial gradient back through the transpose of the down-sampling, which is linear - the final all-reduce sums the
        ranks' parts.
        `comm` (a Communicator): both collectives go through the C ABI's RCCL communicator (nst_comm_allreduce_sum on
        the job's stream; gradient and loss row are ONE packed buffer, as in nst_opt_shard_levels_comm) and rank / world
        are the communicator's; otherwise through `dist_mod` (torch.distributed: gloo rehearsals, or nccl).
        `blend`: the job's style blend (set_targets_blend) - every entry of style_t is then the LIST of that level's K style
        images; the stripe closure takes its Gram targets from the level's targets, so a blend is honoured.  Style layer
        weights other than 1 are not (nst_window_* returns NST_E_STATE under them): ValueError."""
        from . import sharding
        if comm is not None:
            rank, world = comm.rank, comm.world
        elif dist_mod is None:
            import torch.distributed as dist_mod
        e = self.engine
        if any(e.guidance(l)[0] for l in range(e.levels)):
            raise ValueError("content_regions / style_regions cannot be combined with stripe sharding")
        if e.layer_weights != _style.UNIT_WEIGHTS:
            raise ValueError("the stripe closure implements unit style layer weights only (reset_style_weights())")
        if e.laplacian is not None:
            raise ValueError("laplacian_weight cannot be combined with stripe sharding (reset_laplacian())")
        if getattr(e, "matting", None) is not None:
            raise ValueError("matting_weight cannot be combined with stripe sharding (reset_matting())")
        _gram.check_exclusive(getattr(e, "gram_shift", None), stripes=True)
        _mom.check_exclusive(getattr(e, "moment_loss", None), stripes=True)
        if any(e.anchor(l)[0] > 0 for l in range(e.levels)):
            raise ValueError("a temporal anchor cannot be combined with stripe sharding (clear_anchor())")
        _mrf.check_exclusive(next((st for st in (e.patches_setting(l) for l in range(e.levels)) if st is not None), None), stripes=True)
        _hist.check_exclusive(next((st for st in (e.histograms_setting(l) for l in range(e.levels)) if st is not None), None), stripes=True)
        _remd.check_exclusive(next((st for st in (e.remd_setting(l) for l in range(e.levels)) if st is not None), None), stripes=True)
        _selfsim.check_exclusive(next((st for st in (e.selfsim_setting(l) for l in range(e.levels)) if st is not None), None), stripes=True)
        _xcorr.check_exclusive(next((st for st in (e.xcorr_setting(l) for l in range(e.levels)) if st is not None), None), stripes=True)
        contents = list(content_t) if isinstance(content_t, (list, tuple)) else [content_t]
        styles = list(style_t) if isinstance(style_t, (list, tuple)) else [style_t]
        if blend is not None and styles and isinstance(styles[0], torch.Tensor):
            styles = [styles]                    # one striped level: its K style images
        if e.channels != 3:
            raise NstError("the stripe closure implements RGB only (set_color('rgb'))")
        H, W = e.shape
        nstriped = min(len(contents), len(styles), e.levels)
        plans, stripes = [], []
        for l in range(nstriped):
            plan = sharding.StripePlan(H >> l, world, rank)
            st = StyleEngine(weights, e.device)
            st.configure(1, plan.ext_rows, W >> l)
            if blend is None:
                st.set_targets(0, plan.cut(contents[l]), styles[l].contiguous())
            else:
                st.set_targets_blend(0, plan.cut(contents[l]), styles[l], blend)
            plans.append(plan)
            stripes.append(st)
        self._stripes, self._plans = stripes, plans
        self._stripe, self._plan = stripes[0], plans[0]
        n = 3 * H * W
        self._pack = torch.zeros(n + self.row, dtype=torch.float32, device=e.device)
        self._g = self._pack[:n].view(1, 3, H, W)
        self._l = self._pack[n:]
        count = stripes[0].window_sums_count()
        sums_all = torch.empty(nstriped * count, dtype=torch.float32, device=e.device)
        # the other levels: dealt largest first onto the least-loaded rank (every rank carries an equal stripe of the
        # striped levels); a striped level is nobody's in the level mask (its stripes are added here)
        mask = 0
        for l in sharding.deal_levels(range(nstriped, e.levels), world)[rank]:
            mask |= 1 << l

        def hook(_user):
            x, (cw, sw, tvw) = self._x, self._w
            imgs, cuts = [x], []
            for l in range(nstriped):
                if l > 0:
                    imgs.append(e.bicubic_half(imgs[-1]))               # x_l = D x_{l-1}, whole image
                xs = plans[l].cut(imgs[l])
                cuts.append(xs)
                stripes[l].window_begin(xs, plans[l].row0, plans[l].rows, H >> l, sums_all[l * count:(l + 1) * count])
            if comm is not None:
                comm.allreduce_sum(sums_all)
            else:
                dist_mod.all_reduce(sums_all, op=dist_mod.ReduceOp.SUM, group=group)
            for l in range(nstriped):
                gxs, row = stripes[l].window_end(cuts[l], plans[l].row0, plans[l].rows, H >> l, cw, sw, tvw,
                                                 sums_all[l * count:(l + 1) * count])
                if l == 0:
                    plans[0].add_into(self._g, gxs)
                else:
                    gl = torch.zeros_like(imgs[l])
                    plans[l].add_into(gl, gxs)
                    for k in range(l, 0, -1):                           # back through the down-sampling chain: D^T
                        gl = e.bicubic_half_backward(gl, H >> (k - 1), W >> (k - 1))
                    self._g += gl
                if rank == 0:                  # every rank holds the same row of a striped level: one contributor
                    self._l[4 * l:4 * l + 4] = row[0:4]
            if comm is not None:
                comm.allreduce_sum(self._pack)
                sharding.reform_total(self._l)
            else:
                sharding.allreduce_closure(self._g, self._l, dist_mod, group)

        self._hook = _lib.REDUCE_HOOK(hook)
        _lib.check(e.ctx, e.lib.nst_opt_shard_levels(self.h, mask, _ptr(self._g), _ptr(self._l), self._hook, None),
                   "nst_opt_shard_levels")

    def step(self, x: torch.Tensor, cw: float, sw: float, tvw: float, want_losses: bool = True):
        """One optimizer.step(closure). Returns (StepInfo, rows[closures, 4*levels+1] or None)."""
        e = self.engine
        _chk_dev(x, e.device)
        self._x, self._w = x, (cw, sw, tvw)          # what a stripe hook evaluates (x is updated in place)
        info = StepInfo()
        ptr = C.c_void_p(self._rows.ctypes.data) if want_losses else C.c_void_p(0)
        _lib.check(e.ctx, e.lib.nst_opt_step(self.h, _ptr(x), cw, sw, tvw, ptr, self.cap, C.byref(info),
                                             _stream(e.device)), "nst_opt_step")
        rows = self._rows[:min(info.closures, self.cap)].copy() if want_losses else None
        return info, rows

    def close(self):
        if getattr(self, "h", None) and getattr(self.engine, "ctx", None):
            self.engine.lib.nst_opt_destroy(self.h)
        self.h = None
        for st in getattr(self, "_stripes", ()):       # the stripe engines of shard_stripes
            st.close()
        self._stripes = []

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Communicator:
    """nst_comm: an RCCL communicator behind the C ABI (one rank per GPU).  `id_bytes`: the NST_COMM_ID_BYTES of
    `Communicator.unique_id()` made on rank 0 and handed to every rank (e.g. with torch.distributed.broadcast_object_list
    over gloo, or a file)."""

    def __init__(self, device: int, rank: int, world: int, id_bytes: bytes):
        self.lib = _lib.load()
        if len(id_bytes) != _lib.NST_COMM_ID_BYTES:
            raise NstError("communicator id must be NST_COMM_ID_BYTES long")
        buf = C.create_string_buffer(bytes(id_bytes), _lib.NST_COMM_ID_BYTES)
        h = C.c_void_p()
        _lib.check(None, self.lib.nst_comm_create(int(device), rank, world, buf, C.byref(h)), "nst_comm_create")
        self.h, self.rank, self.world, self.device = h, rank, world, torch.device("cuda", int(device))

    @staticmethod
    def unique_id() -> bytes:
        lib = _lib.load()
        buf = C.create_string_buffer(_lib.NST_COMM_ID_BYTES)
        _lib.check(None, lib.nst_comm_unique_id(buf), "nst_comm_unique_id")
        return buf.raw

    def allreduce_sum(self, t: torch.Tensor) -> None:
        _chk_dev(t, self.device)
        _lib.check(None, self.lib.nst_comm_allreduce_sum(self.h, _ptr(t), t.numel(), _stream(self.device)),
                   "nst_comm_allreduce_sum")

    def info(self):
        """(rank, world, all-reduce calls so far, bytes carried)."""
        r, w, n, b = C.c_int(), C.c_int(), C.c_long(), C.c_double()
        _lib.check(None, self.lib.nst_comm_info(self.h, C.byref(r), C.byref(w), C.byref(n), C.byref(b)), "nst_comm_info")
        return r.value, w.value, n.value, b.value

    def close(self):
        if getattr(self, "h", None):
            self.lib.nst_comm_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
