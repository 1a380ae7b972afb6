"""Job driver and optimisation loop with the reference's public surface
(neural_style_transfer.py:32-439), re-implemented on the MI355X HIP engine.

What changed underneath: the reference builds an autograd graph per closure out of torch ops and
lets torch.optim walk it; here one `nst_opt_step` call runs the whole `optimizer.step(closure)` -
pyramid down-sampling, VGG19 forward of every level, Gram/content/TV losses, the hand-written
backward and the Adam / L-BFGS update - inside libnst_hip.so on the device-resident pixel buffer.
There is no CPU path: without a GPU and the built extension these entry points raise."""
from __future__ import annotations

import asyncio
import os
import traceback
from typing import List, Optional

import numpy as np
import torch

from . import device_image, host_image, math_utils
from . import taps as _taps
from .engine import PixelOptimizer, StyleEngine
from .neural_nets import lease_engine, return_engine, shared_engine
from .pooling_modes import check_pooling
from . import style_modes as _style
from . import regions as _regions
from . import gram_modes as _gram
from . import laplacian_modes as _lap
from . import matting_modes as _mat
from . import moment_modes as _mom

# ImageNet statistics (reference :22-23)
IMAGENET_MEAN_255 = [123.675, 116.28, 103.53]
IMAGENET_STD_NEUTRAL = [1, 1, 1]

# how many closure evaluations LBFGS may spend per step; 1 = torch 2.10 semantics of the reference's
# constructor arguments (almost every trial step is rejected), 26 = the line search older torch builds
# performed.  Environment NST_LBFGS_MAX_EVAL overrides it at import; see INTEGRATION.md.
LBFGS_MAX_EVAL = int(os.environ.get("NST_LBFGS_MAX_EVAL", "1"))
VERBOSE = False


class ContentStylePair:
    """content = (name, HWC float32 RGB [0,1] image), style = (name, image)."""

    def __init__(self, content, style):
        self.content = content
        self.style = style


def prepare_img(img, device):
    """HWC [0,1] -> (1,3,H,W) `*255 - ImageNet mean` on `device` (reference :375-383)."""
    dev = torch.device(device)
    hwc = torch.from_numpy(np.ascontiguousarray(img, dtype=np.float32)).to(dev)
    return shared_engine(dev).prepare_img(hwc)


def unprepare_img(img: torch.Tensor):
    """(1,3,H,W) -> HWC float32 numpy, `(+mean)/255`, not clipped (reference :386-393)."""
    t = img.detach().contiguous()
    return shared_engine(t.device).unprepare_img(t).cpu().numpy()


class RepresentationBuilder:
    """Content / style representations of an image from the network's six feature maps."""

    def __init__(self, image, neural_net):
        self.__features = neural_net(image)

    def build_content(self, feature_map_indices):
        listed = isinstance(feature_map_indices, list)
        idx = feature_map_indices if listed else [feature_map_indices]
        rep = [x.squeeze(0) for i, x in enumerate(self.__features) if i in idx]
        return rep if listed else rep[0]

    def build_style(self, feature_map_indices):
        listed = isinstance(feature_map_indices, list)
        idx = feature_map_indices if listed else [feature_map_indices]
        rep = [math_utils.gram_matrix(x) for i, x in enumerate(self.__features) if i in idx]
        return rep if listed else rep[0]


class LossBuilder:
    """Loss of one pyramid level. `build(x)` returns (total, content, style, tv) as device scalars
    evaluated by the fused HIP closure (they carry no autograd graph; the loop obtains the
    gradient from the same closure call)."""

    def __init__(self, content_feature_maps_index, style_feature_maps_indices, target_content_image,
                 target_style_image, neural_net, content_weight, style_weight, tv_weight):
        # any taps of the reference's six maps (ValueError where the reference would fail or silently ignore an index:
        # taps.normalize_taps); the flavour (use_relu) and the pooling are the network's
        use_relu = bool(getattr(neural_net, "use_relu", True))
        pooling = check_pooling(getattr(neural_net, "pooling", "max"))
        taps = _taps.normalize_taps(content_feature_maps_index, style_feature_maps_indices, use_relu)
        self.__weights = (float(content_weight), float(style_weight), float(tv_weight))
        c = target_content_image
        # a context from the per-GPU pool (the weights are uploaded once, not per LossBuilder); it goes back when this
        # object is collected
        self.__engine = lease_engine(c.device)
        self.__engine.configure(1, c.shape[-2], c.shape[-1])
        self.__engine.set_taps(*taps, use_relu=use_relu)
        if pooling != "max":
            self.__engine.set_pooling(pooling)
        self.__targets = (c.contiguous(), target_style_image.contiguous())
        self.__engine.set_targets(0, *self.__targets)

    def set_laplacian(self, laplacian_weight=None, laplacian_pool=_lap.DEFAULT_POOL):
        """Extension: the Laplacian loss (Li et al. 2017) as one more term of `build` - weight(s) gamma_k and pool size(s)
        p_k, each a number or a sequence of up to four; the level total gains sum_k gamma_k lap_k (see
        nst_job_set_laplacian in include/nst_hip.h).  None, 0 or all-zero weights switch it off.  ValueError for a malformed
        setting or an image too small for a pool size."""
        entries = _lap.normalize_laplacian(laplacian_weight, laplacian_pool)
        if entries is not None:
            _lap.check_levels(entries[0], 1, *self.__engine.shape)
        if entries is None and self.__engine.laplacian is None:
            return
        if entries is None:
            self.__engine.reset_laplacian()
        else:
            self.__engine.set_laplacian(*entries)
        self.__engine.set_targets(0, *self.__targets)       # (the setting drops them: the Laplacian targets are made with them)

    def set_matting(self, matting_weight=None, matting_epsilon=_mat.DEFAULT_EPSILON):
        """Extension: the matting term (Luan et al. 2017) as one more term of `build` - the level total gains
        matting_weight * mat, the quadratic form of the content's matting Laplacian on the image (see nst_job_set_matting in
        include/nst_hip.h).  None or 0 switches it off.  ValueError for a malformed setting."""
        setting = _mat.normalize_matting(matting_weight, matting_epsilon)
        if setting is None and self.__engine.matting is None:
            return
        if setting is None:
            self.__engine.reset_matting()
        else:
            self.__engine.set_matting(*setting)
        self.__engine.set_targets(0, *self.__targets)       # (the setting drops them: the guide is made with them)

    def set_gram_shift(self, gram_shift=None):
        """Extension: the Gram statistic of the style term of `build` - activation-shifted (Novak & Nikulin 2016) or
        mean-centred (the covariance; Li et al. 2017) per feature map: None or 0 (the plain Gram), a number (that shift on
        every map), "mean" (every map centred), six entries, or a dict {map index or name: number or "mean"} (see
        nst_job_set_gram_shift in include/nst_hip.h).  ValueError for a malformed setting."""
        setting = _gram.normalize_gram_shift(gram_shift)
        if setting is None and self.__engine.gram_shift is None:
            return
        if setting is None:
            self.__engine.reset_gram_shift()
        else:
            self.__engine.set_gram_shift(*setting)
        self.__engine.set_targets(0, *self.__targets)       # (the setting drops them: the Gram targets are made with the statistic)

    def set_moments(self, moment_weight=None, moment_terms="both", moment_epsilon=_mom.DEFAULT_EPSILON):
        """Extension: the moment loss (Li et al. 2017; Huang & Belongie 2017) as one more term of `build` - the level total
        gains sum_i w_i (mean_i + std_i), the mean squared differences of the channel means and deviations of style map i
        from the style's (see nst_job_set_moments in include/nst_hip.h).  `moment_weight`: None or 0 (off), a number (on
        every style map of this builder), six numbers, or a dict {map index or name: number}; `moment_terms`: "both", "mean"
        or "std".  ValueError for a malformed setting or a positive weight on a map that is not a style map."""
        setting = _mom.normalize_moments(moment_weight, moment_terms, moment_epsilon, style_indices=self.__engine.taps[1],
                                         use_relu=self.__engine.taps[2])
        if setting is None and self.__engine.moment_loss is None:
            return
        if setting is None:
            self.__engine.reset_moments()
        else:
            self.__engine.set_moments(*setting)
        self.__engine.set_targets(0, *self.__targets)       # (the setting drops them: the moment targets are made with them)

    def __del__(self):
        try:
            return_engine(self.__engine)
        except Exception:
            pass

    def build(self, optimizing_img):
        cw, sw, tvw = self.__weights
        _, losses = self.__engine.closure(optimizing_img.detach().contiguous(), cw, sw, tvw)
        return losses[0], losses[1], losses[2], losses[3]


class _DeviceJob:
    """Everything one job owns on the GPU: the engine (targets, workspace), the optimiser (Adam moments / L-BFGS
    history), the job's HIP stream, the side stream and the two pinned host buffers of the per-step yield.
    `NeuralStyleTransfer.process` drives it through four calls - step (pool thread), snapshot, image, close - and is
    otherwise plain asyncio, so the hand-over and tear-down ordering can be tested with a fake in its place
    (`_make_job`, tests/test_host_api.py)."""

    def __init__(self, device, optimizer_name, style_imgs, content_imgs, init_img, lr_start, taps=None, color=None,
                 pooling=None, style_weights=None, blend=None, regions=None, laplacian=None, gram_shift=None, matting=None, moments=None):
        self.dev = dev = device
        self.optimizer = None
        self.luminance = color == "luminance"   # the optimised image is u = 255 Y; the yield puts the content's I, Q back
        self.engine = lease_engine(dev)
        h0, w0 = init_img.shape[:2]
        # Every job runs on a HIP stream of its own: the jobs that share a GPU (`config.simultaneous_tasks_count`
        # per GPU, as in the reference) then overlap on the device - one job's launch tails, host round trips and
        # HBM-bound kernels run under the other's MFMA-bound ones - instead of queueing behind each other on the
        # default stream.  The current stream is per THREAD and the jobs' coroutines share the event-loop thread, so
        # it is set around synchronous sections only, never across an await.
        self.job_stream = torch.cuda.Stream(device=dev)
        self.job_stream.wait_stream(torch.cuda.current_stream(dev))     # the caller built the input images there
        self.copy_stream = torch.cuda.Stream(device=dev)
        try:
            engine = self.engine

            def prepared(img):      # numpy HWC (reference) or a device HWC tensor built by device_image
                if isinstance(img, torch.Tensor):
                    return engine.prepare_img(img.to(dev).contiguous())
                return prepare_img(img, dev)

            def on_device(img):
                if isinstance(img, torch.Tensor):
                    return img.to(dev).contiguous()
                return torch.from_numpy(np.ascontiguousarray(img, dtype=np.float32)).to(dev)

            with torch.cuda.stream(self.job_stream):
                engine.configure(len(content_imgs), h0, w0)
                if taps is not None:                # (content index, style indices, use_relu), normalised
                    engine.set_taps(*taps)
                if pooling is not None:             # "avg": average pooling in the feature network
                    engine.set_pooling(pooling)
                if style_weights is not None:       # six per-layer style weights, checked against the taps
                    engine.set_style_weights(style_weights)
                if laplacian is not None:           # (pools, weights) of the Laplacian loss, normalised
                    engine.set_laplacian(*laplacian)
                if matting is not None:             # (gamma, epsilon) of the matting term, normalised
                    engine.set_matting(*matting)
                if gram_shift is not None:         # (shift[6], center_mask) of the Gram statistic, normalised
                    engine.set_gram_shift(*gram_shift)
                if moments is not None:            # (mean_w[6], std_w[6], epsilon) of the moment loss, normalised
                    engine.set_moments(*moments)
                # blend = (per-level image lists of the extra styles, K x 6 matrix): style 0 is style_imgs
                all_styles = [style_imgs] + (list(blend[0]) if blend is not None else [])
                if self.luminance:
                    # luminance-only transfer: content targets 255 Y(content), style targets 255 (alpha Y(style) + beta)
                    # with the style luminance matched to the content's (statistics of the top level), u0 = 255 Y(init)
                    engine.set_color("luminance")
                    self.content_top = on_device(content_imgs[0])
                    # (every style image is matched to the content's luminance on its own, by its top level's statistics)
                    ab = [device_image.luminance_params(engine, self.content_top, on_device(lv[0])) for lv in all_styles]
                    content_t = lambda img: engine.luminance(on_device(img))                      # noqa: E731
                    style_t = lambda img, k=0: engine.luminance(on_device(img), *ab[k])           # noqa: E731
                else:
                    content_t = prepared
                    style_t = lambda img, k=0: prepared(img)                                      # noqa: E731
                for lvl, (c_img, s_img) in enumerate(zip(content_imgs, style_imgs)):
                    if tuple(c_img.shape[:2]) != engine.level_shape(lvl):
                        raise ValueError(f"content level {lvl} is {tuple(c_img.shape[:2])}, expected {engine.level_shape(lvl)}")
                    if regions is not None:
                        # regions = (per-level content planes, per-level style planes, region weights), host float32 stacks
                        engine.set_guidance(lvl, torch.from_numpy(regions[0][lvl]).to(dev), regions[2])
                        engine.set_targets_guided(lvl, content_t(c_img), style_t(s_img), torch.from_numpy(regions[1][lvl]).to(dev))
                    elif blend is None:
                        engine.set_targets(lvl, content_t(c_img), style_t(s_img))
                    else:
                        engine.set_targets_blend(lvl, content_t(c_img), [style_t(lv[lvl], k) for k, lv in enumerate(all_styles)],
                                                 blend[1])
                self.x = content_t(init_img) if self.luminance else prepared(init_img)
                self.optimizer = PixelOptimizer(engine, optimizer_name, lr_start, LBFGS_MAX_EVAL)
            # Per-step yield (reference :207-208): the image is un-prepared into its own device buffer, copied to
            # pinned host memory on a side stream, and the NEXT optimiser step is started before that copy is
            # awaited, so the 4*3*H*W-byte D2H hides under the next closures.
            self.host = [torch.empty((h0, w0, 3), dtype=torch.float32, pin_memory=True) for _ in range(2)]
        except BaseException:
            self.close()
            raise

    def step(self, cw, sw, tvw):
        """One optimizer.step(closure) (nst_opt_step).  Runs on a pool thread, whose current stream is its own."""
        with torch.cuda.stream(self.job_stream):
            return self.optimizer.step(self.x, cw, sw, tvw, want_losses=True)

    def snapshot(self, k):
        """Un-prepare the current image on the job's stream (ordered BEFORE the next step, which the caller starts
        after this returns) and start its D2H into host buffer k on the side stream.  Returns a callable that blocks
        until the copy has landed."""
        with torch.cuda.device(self.dev), torch.cuda.stream(self.job_stream):
            if self.luminance:
                snap = self.engine.luminance_recombine(self.x, self.content_top)
            else:
                snap = self.engine.unprepare_img(self.x)
            ready = torch.cuda.Event()
            ready.record()
            with torch.cuda.stream(self.copy_stream):
                self.copy_stream.wait_event(ready)
                self.host[k].copy_(snap, non_blocking=True)
                snap.record_stream(self.copy_stream)
                done = torch.cuda.Event()
                done.record()
        return done.synchronize

    def image(self, k):
        return self.host[k].numpy().copy()

    def close(self):
        """The optimiser goes first (its curvature history alone is up to 200 x 12*H*W bytes), then the engine it was
        created on.  The caller guarantees that no step is running (process() drains the worker thread first)."""
        if self.optimizer is not None:
            self.optimizer.close()
            self.optimizer = None
        self.job_stream.synchronize()
        self.copy_stream.synchronize()
        return_engine(self.engine)             # back to the per-GPU pool: the next job re-uses its uploaded weights


def _make_job(device, optimizer_name, style_imgs, content_imgs, init_img, lr_start, taps=None, color=None, pooling=None,
              style_weights=None, blend=None, regions=None, laplacian=None, gram_shift=None, matting=None, moments=None):
    return _DeviceJob(device, optimizer_name, style_imgs, content_imgs, init_img, lr_start, taps, color, pooling,
                      style_weights, blend, regions, laplacian, gram_shift, matting, moments)


async def _drain(step_future):
    """Returns when the WORKER THREAD has left the optimiser step behind `step_future` (the asyncio future
    run_in_executor returned).  Every await on that future goes through asyncio.shield, so cancelling the task never
    cancels the future itself - a cancelled run_in_executor future says nothing about its thread, which would go on
    inside nst_opt_step while the clean-up frees the optimiser and the engine under it.  A CancelledError that arrives
    while waiting is kept and returned for the caller to re-raise after the clean-up."""
    cancelled = None
    while not step_future.done():
        try:
            await asyncio.shield(step_future)
        except asyncio.CancelledError as e:
            if not step_future.done():
                cancelled = e                    # the task was cancelled (again); the thread is still in the step
        except BaseException:
            pass                                 # the step's own failure: the future is done
    if not step_future.cancelled():
        step_future.exception()                  # retrieved: an abandoned step must not warn at garbage collection
    return cancelled


class NeuralStyleTransfer:
    """The optimisation loop (reference :115-208)."""

    def __init__(self, device, model_name, style_imgs, optimizer_name):
        self.__device = torch.device(device)
        self.__model_name = model_name
        self.__style_imgs = style_imgs
        self.__optimizer_name = optimizer_name
        self.__taps = None                       # None: the reference's feature maps
        self.__color = None                      # set_preserve_color
        self.__pooling = "max"                   # set_pooling
        self.__layer_weights = None              # set_style_layer_weights (None: w = 1 on every map)
        self.__blend = None                      # set_style_blend: (extra style levels, blend as given)
        self.__regions = None                    # set_regions: (content stack, style stack, region weights)
        self.__laplacian = None                  # set_laplacian: (pools, weights)
        self.__matting = None                    # set_matting: (gamma, epsilon)
        self.__gram_shift = None               # set_gram_shift: (shift[6], center_mask)
        self.__moments = None                    # set_moments: (moment_weight, moment_terms, moment_epsilon) as given

    def set_feature_maps(self, content_layer=None, style_layers=None, use_relu=True):
        """Extension: the feature maps the losses of the next `process` read - a content map and a set of style maps of
        Vgg19.layer_names, as indices 0..5 or names of the `use_relu` flavour (None: the reference's content 4, style
        [0, 1, 2, 3, 5]).  ValueError for an empty style set, an index out of range or a content map that is not one
        index or name."""
        content, style = _taps.normalize_taps(content_layer, style_layers, use_relu)
        self.__taps = None if _taps.is_default(content, style, use_relu) else (content, style, use_relu)

    def set_preserve_color(self, mode=None):
        """Extension: keep the content image's colours (Gatys, Bethge, Hertzmann & Shechtman 2016) in the next `process`.
        None: the reference's behaviour.  "luminance": the job optimises the luminance u = 255 Y only, against the content
        luminance and the style luminance matched to the content's mean and deviation; every yielded image is
        YIQ^-1 (u / 255, I, Q of content level 0).  "histogram": `process` recolours the style levels with the affine map
        that gives the top style level the top content level's pixel mean and covariance, then runs the RGB job
        (neural_style_transfer() recolours before it builds the initial image and hands the recoloured levels over).
        ValueError for any other value."""
        self.__color = host_image.check_preserve_color(mode)

    def set_pooling(self, mode="max"):
        """Extension: the pooling of the feature network in the next `process` - "max" (the reference's torchvision vgg19)
        or "avg": every 2x2 max-pool replaced by a 2x2 average pool (Gatys, Ecker & Bethge 2016, section 2).  ValueError
        for any other value."""
        self.__pooling = check_pooling(mode)

    def set_style_layer_weights(self, weights=None):
        """Extension: per-layer style weights (the w_l of Gatys, Ecker & Bethge 2016) of the next `process`: the style term
        of a level becomes (sum_i w_i MSE_i) / nstyle.  `weights`: a sequence of 6 numbers >= 0, one per map of
        Vgg19.layer_names, or a dict {map index or name: weight} (maps not named get 1); None: w = 1 everywhere, the
        reference's plain mean.  ValueError for a wrong length, a negative or non-finite entry, an unknown key, or - in
        `process`, where the style set is known - when no map of the style set has a positive weight."""
        w = _style.check_style_layer_weights(weights, style_indices=range(_style.NUM_MAPS))
        self.__layer_weights = None if _style.is_unit(w) else w

    def set_style_blend(self, extra_style_levels=None, blend=None):
        """Extension: more than one style image in the next `process` (jcjohnson's -style_blend_weights; per map, the scale
        control of Gatys et al. 2017).  `extra_style_levels`: a list of per-level image lists, one per extra style, each
        like the constructor's `style_imgs` (style 0 is the constructor's; sizes are each style's own).  `blend`: K numbers
        (the same weight on every map) or a K x 6 array B[k][i] >= 0, K = 1 + the number of extra styles; the Gram target
        of map i is sum_k B[k][i] G_i(style_k) / sum_k B[k][i]; None: an even blend.  None / an empty list: the single
        style.  ValueError for a K that does not match, K > 8, a negative or non-finite entry or - in `process` - a map of
        the style set with an all-zero column."""
        extra = list(extra_style_levels or [])
        if not extra:
            if blend is not None:
                _style.check_style_blend(blend, 1, style_indices=())
            self.__blend = None
            return
        _style.check_style_blend(blend, 1 + len(extra), style_indices=())
        self.__blend = ([list(lv) for lv in extra], blend)

    def set_regions(self, content_regions=None, style_regions=None, region_weights=None):
        """Extension: spatial control (Gatys et al. 2017, guided Gram matrices) in the next `process`: region r of the
        content image takes its style from region r of the style image.  Each argument is an integer label map (H,W) with
        labels 0..R-1 or a float stack (R,H,W) in [0,1], at any resolution (it is resized to every pyramid level of its
        image, nearest neighbour); R <= 4; regions may overlap and need not cover the image.  `region_weights`: R numbers
        >= 0, the weight of each region's term (None: ones).  None, None: no guidance.  ValueError for one of the two
        without the other, mismatched R, values outside [0,1], and - in `process`, where the level sizes are known - a
        region with a mass sum t^2 below 1 on a map of the style set, or guidance together with a style blend."""
        self.__regions = _regions.check_regions(content_regions, style_regions, region_weights)

    def set_laplacian(self, laplacian_weight=None, laplacian_pool=_lap.DEFAULT_POOL):
        """Extension: the Laplacian loss (Li, Xu, Nikolova & He 2017) in the next `process`: a pixel-space term that keeps
        the content's edges.  Per pyramid level and entry k it is gamma_k times the mean squared difference between the
        Laplacian of the p_k x p_k mean-pooled image and that of the pooled content level (nst_job_set_laplacian in
        include/nst_hip.h has the definition).  `laplacian_weight`, `laplacian_pool`: each a number or a sequence of up to
        four (a single weight goes with every pool size); pool sizes are distinct integers in 1..32.  None, 0 or all-zero
        weights: off; zero-weight entries are dropped.  ValueError for a malformed setting and - in `process`, where the
        level sizes are known - for a level too small for a pool size."""
        self.__laplacian = _lap.normalize_laplacian(laplacian_weight, laplacian_pool)

    def set_matting(self, matting_weight=None, matting_epsilon=_mat.DEFAULT_EPSILON):
        """Extension: the photorealism regulariser of Luan, Paris, Shechtman & Bala 2017 in the next `process`: per pyramid
        level matting_weight times the quadratic form of the matting Laplacian of the content level on the level image,
        which is zero where the image is, in every 3x3 window, an affine function of the content's colours
        (nst_job_set_matting in include/nst_hip.h has the definition).  `matting_epsilon` > 0 regularises the windows whose
        colours lie on a line or are constant.  None or 0: off.  ValueError for a malformed setting."""
        self.__matting = _mat.normalize_matting(matting_weight, matting_epsilon)

    def set_gram_shift(self, gram_shift=None):
        """Extension: the Gram statistic of the style term in the next `process` - activation-shifted (Novak & Nikulin 2016:
        G = (F + s)^T (F + s), s = -1 in the paper) or mean-centred (the covariance; Li et al. 2017), per feature map of
        Vgg19.layer_names: None or 0 (the plain Gram), a number (that shift on every map), "mean" (every map centred), six
        entries, or a dict {map index or name: number or "mean"} (the rest 0); nst_job_set_gram_shift in include/nst_hip.h
        has the definition.  ValueError for a non-finite number, another string, a wrong length or an unknown map, and - in
        `process` - together with regions."""
        self.__gram_shift = _gram.normalize_gram_shift(gram_shift)

    def set_moments(self, moment_weight=None, moment_terms="both", moment_epsilon=_mom.DEFAULT_EPSILON):
        """Extension: the moment loss in the next `process` - the "BN statistics matching" of Li et al. 2017 and the style
        loss of Huang & Belongie 2017: per pyramid level sum_i w_i (mean_i + std_i), the mean squared differences of the
        channel means and of the channel deviations sqrt(var + epsilon) of style map i from the style's
        (nst_job_set_moments in include/nst_hip.h has the definition).  `moment_weight`: None or 0 (off), a number (that
        weight on every style map of the job), six numbers by map index of Vgg19.layer_names, or a dict {map index or name:
        number} (the rest 0); `moment_terms`: "both", "mean" or "std"; `moment_epsilon` > 0.  ValueError for a malformed
        setting and - in `process`, where the style set is known - for a positive weight on a map that is not a style map,
        or together with regions."""
        off = _mom.normalize_moments(moment_weight, moment_terms, moment_epsilon, style_indices=range(_mom.NUM_MAPS)) is None
        self.__moments = None if off else (moment_weight, moment_terms, moment_epsilon)

    async def process(self, content_imgs, init_img, lr_start, iters_num, content_weight, style_weight, tv_weight,
                      init_img_name):
        # validates the model name exactly as the reference does (ValueError for anything but vgg19)
        math_utils.prepare_model(self.__model_name, self.__device)
        if self.__optimizer_name not in ("adam", "lbfgs"):
            raise RuntimeError("Unknown optimizer")
        if self.__device.type != "cuda":
            raise RuntimeError("the HIP style-transfer engine needs a GPU; no CPU path exists")
        # the style settings against the style set of THIS job, before any GPU work
        style_set = (self.__taps or (None, _taps.DEFAULT_STYLE_INDICES))[1]
        layer_weights = blend = None
        if self.__layer_weights is not None:
            layer_weights = _style.check_style_layer_weights(self.__layer_weights, style_indices=style_set)
        if self.__blend is not None:
            for lv in self.__blend[0]:
                if len(lv) != len(self.__style_imgs):
                    raise ValueError(f"an extra style has {len(lv)} levels, the job has {len(self.__style_imgs)}")
            blend = (self.__blend[0], _style.check_style_blend(self.__blend[1], 1 + len(self.__blend[0]), style_indices=style_set))
        if self.__laplacian is not None and len(content_imgs):
            _lap.check_levels(self.__laplacian[0], len(content_imgs), *tuple(content_imgs[0].shape[:2]))
        if self.__matting is not None and len(content_imgs):
            _mat.check_levels(len(content_imgs), *tuple(content_imgs[0].shape[:2]))
        _gram.check_exclusive(self.__gram_shift, self.__regions)
        moments = None
        if self.__moments is not None:
            moments = _mom.normalize_moments(*self.__moments, style_indices=style_set,
                                             use_relu=self.__taps[2] if self.__taps is not None else True)
            _mom.check_exclusive(moments, self.__regions)
        style_imgs = self.__style_imgs
        regions = None
        if self.__regions is not None:
            # resized to every level of the content and of the style pyramid and checked for their masses, on the host
            _regions.check_exclusive(self.__regions, blend[0] if blend is not None else None)
            c_stack, s_stack, lam = self.__regions
            regions = (_regions.level_planes(c_stack, [tuple(c.shape[:2]) for c in content_imgs], style_set, "content_regions"),
                       _regions.level_planes(s_stack, [tuple(s.shape[:2]) for s in style_imgs], style_set, "style_regions"), lam)
        if self.__color == "histogram":
            # every style's levels recoloured with its own statistics (those of its top level)
            setup = shared_engine(self.__device)

            def up(img):
                t = img if isinstance(img, torch.Tensor) else device_image.upload(setup, img)
                return t.to(self.__device).contiguous()

            content_top = up(content_imgs[0])
            style_imgs = device_image.recolor_histogram(setup, content_top, [up(s) for s in style_imgs])
            if blend is not None:
                blend = ([device_image.recolor_histogram(setup, content_top, [up(s) for s in lv]) for lv in blend[0]], blend[1])
        extra = {}
        if self.__taps is not None:
            extra["taps"] = self.__taps
        if self.__color == "luminance":
            extra["color"] = "luminance"
        if self.__pooling != "max":
            extra["pooling"] = self.__pooling
        if layer_weights is not None:
            extra["style_weights"] = layer_weights
        if blend is not None:
            extra["blend"] = blend
        if regions is not None:
            extra["regions"] = regions
        if self.__laplacian is not None:
            extra["laplacian"] = self.__laplacian
        if self.__matting is not None:
            extra["matting"] = self.__matting
        if self.__gram_shift is not None:
            extra["gram_shift"] = self.__gram_shift
        if moments is not None:
            extra["moments"] = moments
        job = _make_job(self.__device, self.__optimizer_name, style_imgs, content_imgs, init_img, lr_start, **extra)
        cw, sw, tvw = float(content_weight), float(style_weight), float(tv_weight)
        loop = asyncio.get_running_loop()

        def one_step():
            try:
                return job.step(cw, sw, tvw)
            except Exception:
                traceback.print_exc()
                raise

        step, k = 0, 0
        pending = loop.run_in_executor(None, one_step) if step < iters_num else None
        cancelled = None
        try:
            while pending is not None:
                info, rows = await asyncio.shield(pending)
                pending = None
                step = info.total_closures
                if VERBOSE:
                    for r in rows:
                        print(f"{self.__optimizer_name} | {init_img_name} | lr={info.lr:.4f} | total loss={r[-1]:.3e}")
                copied = job.snapshot(k)                 # ordered before the next step on the job's stream
                if step < iters_num:
                    pending = loop.run_in_executor(None, one_step)
                await loop.run_in_executor(None, copied)
                img = job.image(k)
                k ^= 1
                yield img, step
        finally:
            # Normal end, a consumer that stops early (aclose / GeneratorExit at the yield), a cancelled task or a
            # failed step all come through here.  First the worker thread itself is waited for (not the cancellable
            # future around it), then the job's device objects go.
            if pending is not None:
                cancelled = await _drain(pending)
            job.close()
            if cancelled is not None:
                raise cancelled


async def resize(img, level):
    """Image resized for pyramid level `level`: short edge 256 * 2**level, bicubic, always from the
    original (reference :211-226)."""
    return host_image.resize_to_level(np.array(img, copy=True), level)


gaussian_mask = host_image.gaussian_mask
make_style_noise = host_image.make_style_noise


async def neural_style_transfer(content_n_style: ContentStylePair,
                                content_weight, style_weight, tv_weight,
                                optimizer, model, init_method,
                                iters_num, levels_num, noise_factor, noise_levels, noise_levels_central_amplitude,
                                noise_levels_peripheral_amplitude, noise_levels_dispersion, device=None, *,
                                content_layer=None, style_layers=None, use_relu=True, preserve_color=None,
                                pooling="max", extra_styles=None, style_blend=None, style_layer_weights=None,
                                content_regions=None, style_regions=None, region_weights=None,
                                laplacian_weight=None, laplacian_pool=_lap.DEFAULT_POOL, gram_shift=None,
                                matting_weight=None, matting_epsilon=_mat.DEFAULT_EPSILON,
                                moment_weight=None, moment_terms="both", moment_epsilon=_mom.DEFAULT_EPSILON):
    """Async generator yielding (percent, HWC float32 image) after every optimiser step
    (reference :229-372). `device` (extension): the GPU to run on; default = current.  `content_layer`,
    `style_layers`, `use_relu` (extension): the feature maps the losses read, see NeuralStyleTransfer.set_feature_maps
    (None: the reference's).  `preserve_color` (extension): None, "luminance" or "histogram", see
    NeuralStyleTransfer.set_preserve_color; under "histogram" the style levels are recoloured once, here, and the noise
    map and the "style" initial image are built from the recoloured ones.  `pooling` (extension): "max" or "avg", see
    NeuralStyleTransfer.set_pooling.  `extra_styles` (extension): further style images (HWC float [0,1], any sizes; their
    pyramids are built here), blended with `content_n_style.style` - style 0, which alone feeds the noise map and the
    "style" initial image - by `style_blend`: K numbers or a K x 6 array, see NeuralStyleTransfer.set_style_blend (None: an
    even blend).  `style_layer_weights` (extension): see NeuralStyleTransfer.set_style_layer_weights.  Under
    preserve_color="histogram" every style's levels are recoloured with its own statistics, under "luminance" every
    style's luminance is matched to the content's on its own.  `content_regions`, `style_regions`, `region_weights`
    (extension): spatial control, see NeuralStyleTransfer.set_regions; not with `extra_styles`.  They are validated before
    any GPU work (the masses of the regions on every level included: the level sizes follow from the image sizes).
    `laplacian_weight`, `laplacian_pool` (extension): the Laplacian loss, see NeuralStyleTransfer.set_laplacian (None, 0 or
    all-zero weights: off); validated before any GPU work too, a level too small for a pool size included.  `gram_shift`
    (extension): activation-shifted or mean-centred Gram matrices, see NeuralStyleTransfer.set_gram_shift (None or 0: the
    plain Gram); validated before any GPU work too; not with `content_regions` / `style_regions`.  `matting_weight`,
    `matting_epsilon` (extension): the photorealism regulariser of Luan et al. 2017, see NeuralStyleTransfer.set_matting
    (None or 0: off); validated before any GPU work too.  `moment_weight`, `moment_terms`, `moment_epsilon` (extension): the
    moment loss - channel means and deviations of the style maps matched to the style's - see
    NeuralStyleTransfer.set_moments (None or 0: off); validated before any GPU work too; not with `content_regions` /
    `style_regions`."""
    taps = _taps.normalize_taps(content_layer, style_layers, use_relu)
    host_image.check_preserve_color(preserve_color)
    check_pooling(pooling)
    extra_styles = list(extra_styles) if extra_styles is not None else []
    layer_weights = _style.check_style_layer_weights(style_layer_weights, style_indices=taps[1], use_relu=use_relu)
    if extra_styles or style_blend is not None:
        style_blend = _style.check_style_blend(style_blend, 1 + len(extra_styles), style_indices=taps[1])
    regions = _regions.check_regions(content_regions, style_regions, region_weights)
    _regions.check_exclusive(regions, extra_styles)
    gram_setting = _gram.normalize_gram_shift(gram_shift, use_relu)
    _gram.check_exclusive(gram_setting, regions)
    moment_setting = _mom.normalize_moments(moment_weight, moment_terms, moment_epsilon, style_indices=taps[1], use_relu=use_relu)
    _mom.check_exclusive(moment_setting, regions)
    laplacian = _lap.normalize_laplacian(laplacian_weight, laplacian_pool)
    if laplacian is not None:
        ih, iw = np.shape(content_n_style.content[1])[:2]
        _lap.check_levels(laplacian[0], max(levels_num, 1), *host_image.level_size(ih, iw, max(levels_num - 1, 0)))
    matting = _mat.normalize_matting(matting_weight, matting_epsilon)
    if matting is not None:
        ih, iw = np.shape(content_n_style.content[1])[:2]
        _mat.check_levels(max(levels_num, 1), *host_image.level_size(ih, iw, max(levels_num - 1, 0)))
    if regions is not None:
        for stack, img, what in ((regions[0], content_n_style.content[1], "content_regions"),
                                 (regions[1], content_n_style.style[1], "style_regions")):
            ih, iw = np.shape(img)[:2]
            shapes = [host_image.level_size(ih, iw, lvl) for lvl in range(max(levels_num - 1, 0), -1, -1)]
            _regions.level_planes(stack, shapes, taps[1], what)
    for img in extra_styles:
        if np.ndim(img) != 3 or np.shape(img)[2] != 3:
            raise ValueError(f"extra_styles: expected HWC images with 3 channels, got shape {np.shape(img)}")
    if device is None:
        if not torch.cuda.is_available():
            raise RuntimeError("no GPU visible: the HIP style-transfer engine has no CPU path")
        device = torch.device("cuda", torch.cuda.current_device())
    device = torch.device(device)

    # pyramid + structured-noise initial image, on the device (device_image.py; host_image.py is the
    # host restatement of the same algorithm)
    setup = shared_engine(device)
    content_dev = device_image.upload(setup, content_n_style.content[1])
    style_dev = device_image.upload(setup, content_n_style.style[1])
    content_levels = device_image.pyramid(setup, content_dev, levels_num)
    style_levels = device_image.pyramid(setup, style_dev, levels_num)
    extra_levels = [device_image.pyramid(setup, device_image.upload(setup, img), levels_num) for img in extra_styles]
    style_init = None
    if preserve_color == "histogram":
        style_levels = device_image.recolor_histogram(setup, content_levels[0], style_levels)
        extra_levels = [device_image.recolor_histogram(setup, content_levels[0], lv) for lv in extra_levels]
        style_init = style_levels[0]
    level = max(levels_num - 1, 0)
    init_img, tag = device_image.initial_image(
        setup, init_method, content_dev, style_dev, content_levels[0], style_levels[0], level,
        noise_factor, noise_levels, noise_levels_central_amplitude, noise_levels_peripheral_amplitude,
        noise_levels_dispersion, style_init=style_init)
    init_name = {"random": "random", "content": content_n_style.content[0], "style": content_n_style.style[0]}[tag]

    nst = NeuralStyleTransfer(device, model, style_levels, optimizer)
    nst.set_feature_maps(*taps, use_relu=use_relu)
    nst.set_preserve_color("luminance" if preserve_color == "luminance" else None)   # (histogram: recoloured above)
    nst.set_pooling(pooling)
    nst.set_style_layer_weights(layer_weights)
    nst.set_style_blend(extra_levels, style_blend if extra_levels else None)
    if regions is not None:
        nst.set_regions(regions[0], regions[1], regions[2])
    if laplacian is not None:
        nst.set_laplacian(laplacian[1], laplacian[0])
    if gram_setting is not None:
        nst.set_gram_shift(gram_shift)
    if matting is not None:
        nst.set_matting(*matting)
    if moment_setting is not None:
        nst.set_moments(moment_weight, moment_terms, moment_epsilon)
    lr_start = 10.0
    async for img, cur_iter in nst.process(content_levels, init_img, lr_start, iters_num, content_weight,
                                           style_weight, tv_weight, init_name):
        yield cur_iter / iters_num * 100.0, img
