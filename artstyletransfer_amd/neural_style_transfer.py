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
from . import job_settings as _job
from . import gram_modes as _gram
from . import laplacian_modes as _lap
from . import matting_modes as _mat
from . import moment_modes as _mom
from . import mrf_modes as _mrf
from . import hist_modes as _hist
from . import remd_modes as _remd
from . import selfsim_modes as _selfsim
from . import xcorr_modes as _xcorr

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
        self.__set_term("laplacian", "laplacian", entries)

    def set_matting(self, matting_weight=None, matting_epsilon=_mat.DEFAULT_EPSILON):
        """Extension: the matting term (Luan et al. 2017) as one more term of `build` - the level total gains
        matting_weight * mat, the quadratic form of the content's matting Laplacian on the image (see nst_job_set_matting in
        include/nst_hip.h).  None or 0 switches it off.  ValueError for a malformed setting."""
        self.__set_term("matting", "matting", _mat.normalize_matting(matting_weight, matting_epsilon))

    def set_gram_shift(self, gram_shift=None):
        """Extension: the Gram statistic of the style term of `build` - activation-shifted (Novak & Nikulin 2016) or
        mean-centred (the covariance; Li et al. 2017) per feature map: None or 0 (the plain Gram), a number (that shift on
        every map), "mean" (every map centred), six entries, or a dict {map index or name: number or "mean"} (see
        nst_job_set_gram_shift in include/nst_hip.h).  ValueError for a malformed setting."""
        self.__set_term("gram_shift", "gram_shift", _gram.normalize_gram_shift(gram_shift))

    def set_moments(self, moment_weight=None, moment_terms="both", moment_epsilon=_mom.DEFAULT_EPSILON):
        """Extension: the moment loss (Li et al. 2017; Huang & Belongie 2017) as one more term of `build` - the level total
        gains sum_i w_i (mean_i + std_i), the mean squared differences of the channel means and deviations of style map i
        from the style's (see nst_job_set_moments in include/nst_hip.h).  `moment_weight`: None or 0 (off), a number (on
        every style map of this builder), six numbers, or a dict {map index or name: number}; `moment_terms`: "both", "mean"
        or "std".  ValueError for a malformed setting or a positive weight on a map that is not a style map."""
        setting = _mom.normalize_moments(moment_weight, moment_terms, moment_epsilon, style_indices=self.__engine.taps[1],
                                         use_relu=self.__engine.taps[2])
        self.__set_term("moments", "moment_loss", setting)

    def __set_term(self, name, cached, setting):
        """A loss term of the engine set (`setting`: the arguments of its set_<name>) or switched off (None); `cached` is
        the engine's attribute that says whether it is on."""
        eng = self.__engine
        if setting is None and getattr(eng, cached) is None:
            return
        if setting is None:
            getattr(eng, "reset_" + name)()
        else:
            getattr(eng, "set_" + name)(*setting)
        eng.set_targets(0, *self.__targets)             # (the setting drops them: the term's targets are made with them)

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

    CONSUMES = ("color", "blend", "regions")   # the resolved settings read here; job_settings.apply makes the engine calls of the others

    def __init__(self, device, optimizer_name, style_imgs, content_imgs, init_img, lr_start, settings):
        """`settings`: the dict JobSettings.resolve gave - "taps": (content index, style indices, use_relu); "pooling":
        "avg"; "style_weights": six per-layer weights; "laplacian": (pools, weights); "matting": (gamma, epsilon);
        "gram_shift": (shift[6], center_mask); "moments": (mean_w[6], std_w[6], epsilon); "color": "luminance"; "blend":
        (per-level image lists of the extra styles, K x 6 matrix); "regions": (per-level content planes, per-level style
        planes, region weights)."""
        color, blend, regions = (settings.get(k) for k in self.CONSUMES)
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
                _job.apply(engine, settings)          # (the colour mode last: the planes below are made under it)
                # blend = (per-level image lists of the extra styles, K x 6 matrix): style 0 is style_imgs
                all_styles = [style_imgs] + (list(blend[0]) if blend is not None else [])
                if self.luminance:
                    # luminance-only transfer: content targets 255 Y(content), style targets 255 (alpha Y(style) + beta)
                    # with the style luminance matched to the content's (statistics of the top level), u0 = 255 Y(init)
                    self.content_top = on_device(content_imgs[0])
                    # (every style image is matched to the content's luminance on its own, by its top level's statistics)
                    ab = [device_image.luminance_params(engine, self.content_top, on_device(lv[0])) for lv in all_styles]
                    content_t = lambda img: engine.luminance(on_device(img))                      # noqa: E731
                    style_t = lambda img, k=0: engine.luminance(on_device(img), *ab[k])           # noqa: E731
                else:
                    content_t = prepared
                    style_t = lambda img, k=0: prepared(img)                                      # noqa: E731
                self.style_levels = [(lambda img=s_img: style_t(img)) for s_img in style_imgs]     # set_patch_match: the images the targets are made from
                self.content_levels = [(lambda img=c_img: content_t(img)) for c_img in content_imgs]   # set_self_similarity: likewise
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

    def set_anchor(self, anchor_levels, weight_levels, gamma):
        """The temporal term's anchors and weights of the levels (StyleEngine.set_anchor; None: a level without)."""
        with torch.cuda.device(self.dev), torch.cuda.stream(self.job_stream):
            for lvl, (a, c) in enumerate(zip(anchor_levels, weight_levels)):
                if a is not None:
                    self.engine.set_anchor(lvl, a, c, gamma=gamma)

    def set_patch_match(self, weights, stride, epsilon, levels):
        """The MRF term of the levels (StyleEngine.set_patches; `levels` None: every level): each level gets the style level
        image its targets were made from - recoloured under "histogram", the matched luminance plane under "luminance"."""
        with torch.cuda.device(self.dev), torch.cuda.stream(self.job_stream):
            for lvl, style_of in enumerate(self.style_levels):
                if levels is None or lvl in levels:
                    self.engine.set_patches(lvl, style_of(), weights, stride, epsilon)

    def set_patch_semantics(self, level_planes, weight):
        """The semantic maps of the MRF term's levels (StyleEngine.set_patch_guidance), after set_patch_match: `level_planes`
        per level (content planes (R,h,w), style planes (R,hs,ws)) as host float32 stacks, or None for a level without."""
        with torch.cuda.device(self.dev), torch.cuda.stream(self.job_stream):
            for lvl, planes in enumerate(level_planes):
                if planes is not None:
                    self.engine.set_patch_guidance(lvl, torch.from_numpy(planes[0]).to(self.dev), torch.from_numpy(planes[1]).to(self.dev),
                                                   weight)

    def set_histogram_loss(self, weights, bins, levels):
        """The histogram loss of the levels (StyleEngine.set_histograms; `levels` None: every level): each level gets the style
        level image its targets were made from, as set_patch_match does."""
        with torch.cuda.device(self.dev), torch.cuda.stream(self.job_stream):
            for lvl, style_of in enumerate(self.style_levels):
                if levels is None or lvl in levels:
                    self.engine.set_histograms(lvl, style_of(), weights, bins)

    def set_relaxed_emd(self, weights, strides, epsilon):
        """The relaxed EMD term of the levels (StyleEngine.set_remd; `strides` per level: None for a level without the term, or
        (image strides, style strides) as remd_modes.level_strides makes them): each level gets the style level image its
        targets were made from, as set_patch_match does."""
        with torch.cuda.device(self.dev), torch.cuda.stream(self.job_stream):
            for lvl, style_of in enumerate(self.style_levels):
                if strides[lvl] is not None:
                    self.engine.set_remd(lvl, style_of(), weights, strides[lvl][0], strides[lvl][1], epsilon)

    def set_self_similarity(self, weights, strides, epsilon):
        """The self-similarity term of the levels (StyleEngine.set_selfsim; `strides` per level: None for a level without the
        term, or six strides as selfsim_modes.level_strides makes them): each level gets the content level image its targets
        were made from."""
        with torch.cuda.device(self.dev), torch.cuda.stream(self.job_stream):
            for lvl, content_of in enumerate(self.content_levels):
                if strides[lvl] is not None:
                    self.engine.set_selfsim(lvl, content_of(), weights, strides[lvl], epsilon)

    def set_shifted_gram(self, weights, shifts, carries):
        """The xcorr term of the levels (StyleEngine.set_xcorr; `carries` per level: whether it carries the term, as
        xcorr_modes.level_carries makes it): each level gets the style level image its targets were made from."""
        with torch.cuda.device(self.dev), torch.cuda.stream(self.job_stream):
            for lvl, style_of in enumerate(self.style_levels):
                if carries[lvl]:
                    self.engine.set_xcorr(lvl, style_of(), weights, shifts)

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


def _make_job(device, optimizer_name, style_imgs, content_imgs, init_img, lr_start, **settings):
    unknown = set(settings) - set(_job.KEYS)
    if unknown:
        raise TypeError(f"_make_job() got unexpected setting(s): {sorted(unknown)}")
    return _DeviceJob(device, optimizer_name, style_imgs, content_imgs, init_img, lr_start, settings)


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
        self.settings = _job.JobSettings()       # the optional settings of the next `process`: the set_* below update it
        self.__anchor = None                     # set_anchor: data of the next `process`, not a setting
        self.__patches = None                    # set_patch_match: likewise
        self.__semantics = None                  # set_patch_semantics: likewise
        self.__histograms = None                 # set_histogram_loss: likewise
        self.__remd = None                       # set_relaxed_emd: likewise
        self.__selfsim = None                    # set_self_similarity: likewise
        self.__xcorr = None                      # set_shifted_gram: likewise

    def set_feature_maps(self, content_layer=None, style_layers=None, use_relu=True):
        """Extension: the feature maps the losses of the next `process` read - a content map and a set of style maps of
        Vgg19.layer_names, as indices 0..5 or names of the `use_relu` flavour (None: the reference's content 4, style
        [0, 1, 2, 3, 5]).  ValueError for an empty style set, an index out of range or a content map that is not one
        index or name."""
        self.settings.update(content_layer=content_layer, style_layers=style_layers, use_relu=use_relu)

    def set_preserve_color(self, mode=None):
        """Extension: keep the content image's colours (Gatys, Bethge, Hertzmann & Shechtman 2016) in the next `process`.
        None: the reference's behaviour.  "luminance": the job optimises the luminance u = 255 Y only, against the content
        luminance and the style luminance matched to the content's mean and deviation; every yielded image is
        YIQ^-1 (u / 255, I, Q of content level 0).  "histogram": `process` recolours the style levels with the affine map
        that gives the top style level the top content level's pixel mean and covariance, then runs the RGB job
        (neural_style_transfer() recolours before it builds the initial image and hands the recoloured levels over).
        ValueError for any other value."""
        self.settings.update(preserve_color=mode)

    def set_pooling(self, mode="max"):
        """Extension: the pooling of the feature network in the next `process` - "max" (the reference's torchvision vgg19)
        or "avg": every 2x2 max-pool replaced by a 2x2 average pool (Gatys, Ecker & Bethge 2016, section 2).  ValueError
        for any other value."""
        self.settings.update(pooling=mode)

    def set_style_layer_weights(self, weights=None):
        """Extension: per-layer style weights (the w_l of Gatys, Ecker & Bethge 2016) of the next `process`: the style term
        of a level becomes (sum_i w_i MSE_i) / nstyle.  `weights`: a sequence of 6 numbers >= 0, one per map of
        Vgg19.layer_names, or a dict {map index or name: weight} (maps not named get 1); None: w = 1 everywhere, the
        reference's plain mean.  ValueError for a wrong length, a negative or non-finite entry, an unknown key, or - in
        `process`, where the style set is known - when no map of the style set has a positive weight."""
        self.settings.update(style_layer_weights=weights)

    def set_style_blend(self, extra_style_levels=None, blend=None):
        """Extension: more than one style image in the next `process` (jcjohnson's -style_blend_weights; per map, the scale
        control of Gatys et al. 2017).  `extra_style_levels`: a list of per-level image lists, one per extra style, each
        like the constructor's `style_imgs` (style 0 is the constructor's; sizes are each style's own).  `blend`: K numbers
        (the same weight on every map) or a K x 6 array B[k][i] >= 0, K = 1 + the number of extra styles; the Gram target
        of map i is sum_k B[k][i] G_i(style_k) / sum_k B[k][i]; None: an even blend.  None / an empty list: the single
        style.  ValueError for a K that does not match, K > 8, a negative or non-finite entry or - in `process` - a map of
        the style set with an all-zero column."""
        self.settings.update(extra_styles=[list(lv) for lv in extra_style_levels or []], style_blend=blend)

    def set_regions(self, content_regions=None, style_regions=None, region_weights=None):
        """Extension: spatial control (Gatys et al. 2017, guided Gram matrices) in the next `process`: region r of the
        content image takes its style from region r of the style image.  Each argument is an integer label map (H,W) with
        labels 0..R-1 or a float stack (R,H,W) in [0,1], at any resolution (it is resized to every pyramid level of its
        image, nearest neighbour); R <= 4; regions may overlap and need not cover the image.  `region_weights`: R numbers
        >= 0, the weight of each region's term (None: ones).  None, None: no guidance.  ValueError for one of the two
        without the other, mismatched R, values outside [0,1], and - in `process`, where the level sizes are known - a
        region with a mass sum t^2 below 1 on a map of the style set, or guidance together with a style blend."""
        self.settings.update(content_regions=content_regions, style_regions=style_regions, region_weights=region_weights)

    def set_laplacian(self, laplacian_weight=None, laplacian_pool=_lap.DEFAULT_POOL):
        """Extension: the Laplacian loss (Li, Xu, Nikolova & He 2017) in the next `process`: a pixel-space term that keeps
        the content's edges.  Per pyramid level and entry k it is gamma_k times the mean squared difference between the
        Laplacian of the p_k x p_k mean-pooled image and that of the pooled content level (nst_job_set_laplacian in
        include/nst_hip.h has the definition).  `laplacian_weight`, `laplacian_pool`: each a number or a sequence of up to
        four (a single weight goes with every pool size); pool sizes are distinct integers in 1..32.  None, 0 or all-zero
        weights: off; zero-weight entries are dropped.  ValueError for a malformed setting and - in `process`, where the
        level sizes are known - for a level too small for a pool size."""
        self.settings.update(laplacian_weight=laplacian_weight, laplacian_pool=laplacian_pool)

    def set_matting(self, matting_weight=None, matting_epsilon=_mat.DEFAULT_EPSILON):
        """Extension: the photorealism regulariser of Luan, Paris, Shechtman & Bala 2017 in the next `process`: per pyramid
        level matting_weight times the quadratic form of the matting Laplacian of the content level on the level image,
        which is zero where the image is, in every 3x3 window, an affine function of the content's colours
        (nst_job_set_matting in include/nst_hip.h has the definition).  `matting_epsilon` > 0 regularises the windows whose
        colours lie on a line or are constant.  None or 0: off.  ValueError for a malformed setting."""
        self.settings.update(matting_weight=matting_weight, matting_epsilon=matting_epsilon)

    def set_gram_shift(self, gram_shift=None):
        """Extension: the Gram statistic of the style term in the next `process` - activation-shifted (Novak & Nikulin 2016:
        G = (F + s)^T (F + s), s = -1 in the paper) or mean-centred (the covariance; Li et al. 2017), per feature map of
        Vgg19.layer_names: None or 0 (the plain Gram), a number (that shift on every map), "mean" (every map centred), six
        entries, or a dict {map index or name: number or "mean"} (the rest 0); nst_job_set_gram_shift in include/nst_hip.h
        has the definition.  ValueError for a non-finite number, another string, a wrong length or an unknown map, and - in
        `process` - together with regions."""
        self.settings.update(gram_shift=gram_shift)

    def set_moments(self, moment_weight=None, moment_terms="both", moment_epsilon=_mom.DEFAULT_EPSILON):
        """Extension: the moment loss in the next `process` - the "BN statistics matching" of Li et al. 2017 and the style
        loss of Huang & Belongie 2017: per pyramid level sum_i w_i (mean_i + std_i), the mean squared differences of the
        channel means and of the channel deviations sqrt(var + epsilon) of style map i from the style's
        (nst_job_set_moments in include/nst_hip.h has the definition).  `moment_weight`: None or 0 (off), a number (that
        weight on every style map of the job), six numbers by map index of Vgg19.layer_names, or a dict {map index or name:
        number} (the rest 0); `moment_terms`: "both", "mean" or "std"; `moment_epsilon` > 0.  ValueError for a malformed
        setting and - in `process`, where the style set is known - for a positive weight on a map that is not a style map,
        or together with regions."""
        self.settings.update(moment_weight=moment_weight, moment_terms=moment_terms, moment_epsilon=moment_epsilon)

    def set_anchor(self, anchor_levels=None, weight_levels=None, gamma=0.0):
        """Extension: the temporal consistency term of Ruder, Dosovitskiy & Brox 2016 in the next `process`: per pyramid level
        gamma times the weighted mean squared distance of the level image from an anchor (nst_level_set_anchor in
        include/nst_hip.h has the definition).  `anchor_levels`: per level, top level first, a device tensor of the level
        image's size ((1,3,h,w) prepared; (1,1,h,w) = StyleEngine.luminance(...) under preserve_color "luminance") or None
        for a level without the term; `weight_levels`: per level an (h,w) device tensor in [0,1] or None for ones, or None
        for ones everywhere.  Data of one job, like the content levels - not one of `settings`.  None or gamma 0: off.
        ValueError for a negative or non-finite gamma or lists of differing lengths."""
        g = float(gamma)
        if not np.isfinite(g) or g < 0.0:
            raise ValueError(f"the temporal weight must be finite and >= 0, got {gamma!r}")
        if anchor_levels is None or g == 0.0:
            self.__anchor = None
            return
        anchors = list(anchor_levels)
        weights = list(weight_levels) if weight_levels is not None else [None] * len(anchors)
        if len(weights) != len(anchors):
            raise ValueError(f"{len(anchors)} anchor levels but {len(weights)} weight levels")
        self.__anchor = (anchors, weights, g)

    def set_patch_match(self, weights=None, stride=_mrf.DEFAULT_STRIDE, epsilon=_mrf.DEFAULT_EPSILON, levels=None):
        """Extension: the MRF style term of Li & Wand 2016 (CNNMRF, neural-doodle) in the next `process`: per pyramid level
        sum_i w_i mrf_i, mrf_i the mean squared distance of the 3x3 patches of map i from their nearest neighbours - by
        normalised cross-correlation - among the 3x3 patches of the same map of the level's style image (nst_level_set_patches
        in include/nst_hip.h has the definition).  `weights`: None or 0 (off), a number (that weight on those of relu3_1 and
        relu4_1 that are style maps of the job), six numbers by map index of Vgg19.layer_names, or a dict {map index or name:
        number}; `stride`: the stride of the style patches, 1..8 (the search costs 1 / stride^2); `epsilon` > 0; `levels`:
        None for every level, or the level indices that carry the term (0 = the full resolution).  Data of one job, like the
        anchor - not one of `settings`.  ValueError for a malformed setting and - in `process`, where the style set and the
        level sizes are known - for a positive weight on a map that is not a style map, a weighted map that pools below 3x3
        on a chosen level (on either image), or the term together with regions or several style images."""
        _mrf.normalize_mrf(weights, stride, epsilon, levels)          # (malformed: here and now; the style set comes with `process`)
        off = weights is None or (isinstance(weights, (int, float)) and not isinstance(weights, bool) and weights == 0)
        self.__patches = None if off else (weights, stride, epsilon, levels)

    def set_patch_semantics(self, content_regions=None, style_regions=None, weight=_mrf.DEFAULT_SEMANTIC_WEIGHT):
        """Extension: semantic maps that steer the patch search of the MRF term (Champandard 2016, neural-doodle) in the next
        `process`: a patch of region r of the content prefers style patches of region r of the style - the score of a
        candidate is cos + weight <d, e>, d and e the normalised region descriptors of the two patches
        (nst_level_set_patch_guidance in include/nst_hip.h has the definition).  Each map is an integer label map (H,W) with
        labels 0..R-1 or a float stack (R,H,W) in [0,1], at any resolution (it is resized to every level of its pyramid that
        carries the term, nearest neighbour); R <= 4, equal on the two sides.  `weight`: a finite number >= 0; the cosines
        of post-ReLU maps lie in [0,1], so from 1 on a candidate of the same region always beats one of another region for
        one-hot descriptors, and smaller values trade region for feature similarity.  Data of one job, like set_patch_match
        (which names the maps, the stride and the levels).  None, None or weight 0: off.  ValueError for a malformed
        argument, one map without the other, mismatched R and - in `process` - semantic maps without the MRF term."""
        self.__semantics = _mrf.normalize_semantic(content_regions, style_regions, weight)

    def set_histogram_loss(self, weights=None, bins=_hist.DEFAULT_BINS, levels=None):
        """Extension: the histogram loss of Risser, Wilmot & Barnes 2017 in the next `process`: per pyramid level
        sum_i w_i hist_i, hist_i the mean squared distance of map i from its remap onto the per-channel histograms of the same
        map of the level's style image (nst_level_set_histograms in include/nst_hip.h has the definition).  `weights`: None or
        0 (off), a number (that weight on those of relu1_1 and relu4_1 that are style maps of the job), six numbers by map
        index of Vgg19.layer_names, or a dict {map index or name: number}; `bins`: 2..1024; `levels`: None for every level, or
        the level indices that carry the term (0 = the full resolution).  Data of one job, like set_patch_match - not one of
        `settings`.  ValueError for a malformed setting and - in `process`, where the style set is known - for a positive
        weight on a map that is not a style map, or the term together with regions or several style images."""
        _hist.normalize_hist(weights, bins, levels)          # (malformed: here and now; the style set comes with `process`)
        off = weights is None or (isinstance(weights, (int, float)) and not isinstance(weights, bool) and weights == 0)
        self.__histograms = None if off else (weights, bins, levels)

    def set_relaxed_emd(self, weights=None, samples=_remd.DEFAULT_SAMPLES, epsilon=_remd.DEFAULT_EPSILON, levels=None):
        """Extension: the relaxed EMD style term of Kolkin, Salavon & Shakhnarovich 2019 (STROTSS) in the next `process`: per
        pyramid level sum_i w_i remd_i, remd_i the larger of the two mean cosine distances of the two-way nearest-neighbour
        match between the sampled feature vectors of map i and of the same map of the level's style image (nst_level_set_remd
        in include/nst_hip.h has the definition).  `weights`: None or 0 (off), a number (that weight on those of relu2_1,
        relu3_1 and relu4_1 that are style maps of the job), six numbers by map index of Vgg19.layer_names, or a dict {map
        index or name: number}; `samples`: the most samples per side and map (every map gets the smallest stride that keeps
        to it; the search's cost grows with its square); `epsilon` > 0; `levels`: None for every level, or the level indices
        that carry the term (0 = the full resolution).  Data of one job, like set_patch_match - not one of `settings`.
        ValueError for a malformed setting and - in `process`, where the style set and the sizes are known - for a positive
        weight on a map that is not a style map, a map that needs a stride above 256, or the term together with regions or
        several style images."""
        off = _remd.normalize_remd(weights, samples, epsilon, levels) is None       # (malformed: here and now)
        self.__remd = None if off else (weights, samples, epsilon, levels)

    def set_self_similarity(self, weights=None, samples=_selfsim.DEFAULT_SAMPLES, epsilon=_selfsim.DEFAULT_EPSILON, levels=None):
        """Extension: the self-similarity content term of Kolkin, Salavon & Shakhnarovich 2019 (STROTSS) in the next `process`:
        per pyramid level sum_k w_k selfsim_k, selfsim_k the mean over the sampled positions of map k of the L1 distance between
        the column-normalised matrices of pairwise cosine distances of the image's and of the content's samples
        (nst_level_set_selfsim in include/nst_hip.h has the definition).  It ties the layout to the content's without tying the
        feature values: the term to use with a low content weight beside set_relaxed_emd.  `weights`: None or 0 (off), a number
        (that weight on the job's content map), six numbers by map index of Vgg19.layer_names, or a dict {map index or name:
        number} - any map the job uses may carry one, its content map or a style map; `samples`: 1..4096, the most samples per
        map (every map gets the smallest stride that keeps to it; the term keeps samples x samples arrays; 1024 is the
        paper's count); `epsilon` > 0; `levels`: None for every level, or the level indices that carry the term (0 = the full
        resolution).  Data of one job, like set_relaxed_emd - not one of `settings`.  ValueError for a malformed setting and -
        in `process`, where the taps and the sizes are known - for a positive weight on a map the job does not use, a map that
        needs a stride above 256, or the term together with regions or several style images."""
        off = _selfsim.normalize_selfsim(weights, samples, epsilon, levels) is None       # (malformed: here and now)
        self.__selfsim = None if off else (weights, samples, epsilon, levels)

    def set_shifted_gram(self, weights=None, shifts=_xcorr.DEFAULT_SHIFTS, levels=None):
        """Extension: the long-range style term of Berger & Memisevic 2017 ("xcorr") in the next `process`: per pyramid level
        sum_i w_i xcorr_i, xcorr_i the mean over the shifts d of the mean squared difference between the cross-correlation of
        map i with its copy shifted by d, G_d = (1/Z_d) sum_p F(p + d) F(p)^T, and the same statistic of the level's style
        image (nst_level_set_xcorr in include/nst_hip.h has the definition).  It carries a texture's regular structure - a
        lattice, hatching at a fixed pitch - which every summed statistic is blind to.  `weights`: None or 0 (off), a number
        (that weight on those of relu2_1, relu3_1, relu4_1 that are style maps of the job), six numbers by map index of
        Vgg19.layer_names, or a dict {map index or name: number}; `shifts`: integers k (the axis shifts (k, 0) and (0, k)) or
        pairs (dx, dy), 0..64, at most 16 after expansion, in map pixels; `levels`: None for every level, or the level indices
        that carry the term (0 = the full resolution).  Data of one job, like set_relaxed_emd - not one of `settings`.
        ValueError for a malformed setting and - in `process`, where the taps and the sizes are known - for a positive weight on
        a map that is not a style map, a shift that is not smaller than a weighted map of a carrying level, of either image, or
        the term together with regions or several style images."""
        off = _xcorr.normalize_xcorr(weights, shifts, levels) is None       # (malformed: here and now)
        self.__xcorr = None if off else (weights, shifts, levels)

    async def process(self, content_imgs, init_img, lr_start, iters_num, content_weight, style_weight, tv_weight,
                      init_img_name):
        # validates the model name exactly as the reference does (ValueError for anything but vgg19)
        math_utils.prepare_model(self.__model_name, self.__device)
        if self.__optimizer_name not in ("adam", "lbfgs"):
            raise RuntimeError("Unknown optimizer")
        if self.__device.type != "cuda":
            raise RuntimeError("the HIP style-transfer engine needs a GPU; no CPU path exists")
        # the settings against the style set and the level sizes of THIS job, before any GPU work
        style_imgs = self.__style_imgs
        resolved = self.settings.resolve(lambda: [tuple(c.shape[:2]) for c in content_imgs],
                                         lambda: [tuple(s.shape[:2]) for s in style_imgs], style_levels=len(style_imgs))
        if self.settings["color"] == "histogram":
            # every style's levels recoloured with its own statistics (those of its top level)
            setup = shared_engine(self.__device)

            def up(img):
                t = img if isinstance(img, torch.Tensor) else device_image.upload(setup, img)
                return t.to(self.__device).contiguous()

            content_top = up(content_imgs[0])
            style_imgs = device_image.recolor_histogram(setup, content_top, [up(s) for s in style_imgs])
            if "blend" in resolved:
                extra, blend = resolved["blend"]
                resolved["blend"] = ([device_image.recolor_histogram(setup, content_top, [up(s) for s in lv]) for lv in extra], blend)
        patches = None
        if self.__patches is not None:
            style_set, use_relu = resolved["taps"][1:] if "taps" in resolved else (_taps.DEFAULT_STYLE_INDICES, True)
            patches = _mrf.normalize_mrf(*self.__patches, style_indices=style_set, use_relu=use_relu, levels_num=len(content_imgs))
            _mrf.check_exclusive(patches, regions=resolved.get("regions"), extra_styles=resolved.get("blend"))
            _mrf.check_sizes(patches, [tuple(c.shape[:2]) for c in content_imgs], [tuple(s.shape[:2]) for s in style_imgs])
        semantics = None
        if self.__semantics is not None:
            if patches is None:
                raise ValueError("semantic maps steer the MRF term: set_patch_semantics needs set_patch_match (mrf_weight is off)")
            semantics = _mrf.semantic_level_planes(self.__semantics, [tuple(c.shape[:2]) for c in content_imgs],
                                                   [tuple(s.shape[:2]) for s in style_imgs], patches[3])
        histograms = None
        if self.__histograms is not None:
            style_set, use_relu = resolved["taps"][1:] if "taps" in resolved else (_taps.DEFAULT_STYLE_INDICES, True)
            histograms = _hist.normalize_hist(*self.__histograms, style_indices=style_set, use_relu=use_relu, levels_num=len(content_imgs))
            _hist.check_exclusive(histograms, regions=resolved.get("regions"), extra_styles=resolved.get("blend"))
        remd = None
        if self.__remd is not None:
            style_set, use_relu = resolved["taps"][1:] if "taps" in resolved else (_taps.DEFAULT_STYLE_INDICES, True)
            remd = _remd.normalize_remd(*self.__remd, style_indices=style_set, use_relu=use_relu, levels_num=len(content_imgs))
            _remd.check_exclusive(remd, regions=resolved.get("regions"), extra_styles=resolved.get("blend"))
            remd_strides = _remd.level_strides(remd, [tuple(c.shape[:2]) for c in content_imgs], [tuple(s.shape[:2]) for s in style_imgs])
        selfsim = None
        if self.__selfsim is not None:
            content_i, style_set, use_relu = resolved.get("taps", (_taps.DEFAULT_CONTENT_INDEX, _taps.DEFAULT_STYLE_INDICES, True))
            selfsim = _selfsim.normalize_selfsim(*self.__selfsim, content_index=content_i, style_indices=style_set, use_relu=use_relu,
                                                 levels_num=len(content_imgs))
            _selfsim.check_exclusive(selfsim, regions=resolved.get("regions"), extra_styles=resolved.get("blend"))
            selfsim_strides = _selfsim.level_strides(selfsim, [tuple(c.shape[:2]) for c in content_imgs])
        xcorr = None
        if self.__xcorr is not None:
            _, style_set, use_relu = resolved.get("taps", (_taps.DEFAULT_CONTENT_INDEX, _taps.DEFAULT_STYLE_INDICES, True))
            xcorr = _xcorr.normalize_xcorr(*self.__xcorr, style_indices=style_set, use_relu=use_relu, levels_num=len(content_imgs))
            _xcorr.check_exclusive(xcorr, regions=resolved.get("regions"), extra_styles=resolved.get("blend"))
            xcorr_carries = _xcorr.level_carries(xcorr, [tuple(c.shape[:2]) for c in content_imgs], [tuple(s.shape[:2]) for s in style_imgs])
        if self.__anchor is not None and len(self.__anchor[0]) != len(content_imgs):
            raise ValueError(f"{len(self.__anchor[0])} anchor levels for a job of {len(content_imgs)} levels")
        job = _make_job(self.__device, self.__optimizer_name, style_imgs, content_imgs, init_img, lr_start, **resolved)
        if self.__anchor is not None:        # (data of the job, handed over once the job exists: not one of its settings)
            try:
                job.set_anchor(*self.__anchor)
            except BaseException:
                job.close()
                raise
        if patches is not None:              # (likewise)
            try:
                job.set_patch_match(*patches)
                if semantics is not None:
                    job.set_patch_semantics(semantics, self.__semantics[2])
            except BaseException:
                job.close()
                raise
        if histograms is not None:           # (likewise, after the MRF term)
            try:
                job.set_histogram_loss(*histograms)
            except BaseException:
                job.close()
                raise
        if remd is not None:                 # (likewise, after the histogram loss)
            try:
                job.set_relaxed_emd(remd[0], remd_strides, remd[2])
            except BaseException:
                job.close()
                raise
        if selfsim is not None:              # (likewise, after the relaxed EMD term)
            try:
                job.set_self_similarity(selfsim[0], selfsim_strides, selfsim[2])
            except BaseException:
                job.close()
                raise
        if xcorr is not None:                # (likewise, after the self-similarity term)
            try:
                job.set_shifted_gram(xcorr[0], xcorr[1], xcorr_carries)
            except BaseException:
                job.close()
                raise
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
    kw = dict(content_layer=content_layer, style_layers=style_layers, use_relu=use_relu, preserve_color=preserve_color,
              pooling=pooling, extra_styles=extra_styles, style_blend=style_blend, style_layer_weights=style_layer_weights,
              content_regions=content_regions, style_regions=style_regions, region_weights=region_weights,
              laplacian_weight=laplacian_weight, laplacian_pool=laplacian_pool, gram_shift=gram_shift, matting_weight=matting_weight,
              matting_epsilon=matting_epsilon, moment_weight=moment_weight, moment_terms=moment_terms, moment_epsilon=moment_epsilon)
    job = _transfer_from(content_n_style, content_weight, style_weight, tv_weight, optimizer, model, init_method, iters_num,
                         levels_num, noise_factor, noise_levels, noise_levels_central_amplitude, noise_levels_peripheral_amplitude,
                         noise_levels_dispersion, device=device, start=None, **kw)
    try:
        async for out in job:
            yield out
    finally:
        await job.aclose()       # (a consumer that stops early: the job's device objects go here, not at collection)


def _transfer_from(content_n_style, content_weight, style_weight, tv_weight, optimizer, model, init_method, iters_num, levels_num,
                   noise_factor, noise_levels, noise_levels_central_amplitude, noise_levels_peripheral_amplitude,
                   noise_levels_dispersion, *, device=None, start=None, patches=None, semantics=None, histograms=None, remd=None, selfsim=None,
                   xcorr=None, **keywords):
    """The settings validation of neural_style_transfer() (`keywords`: its keyword-only parameters), here and now - before any
    GPU work, ValueError - and then the job as an async generator, from the `init_method` image or from `start` (_transfer).
    `patches` (patch_match.py): None, or the arguments of NeuralStyleTransfer.set_patch_match, validated here too;
    `semantics`: None, or the arguments of NeuralStyleTransfer.set_patch_semantics, likewise (they need `patches`);
    `histograms` (histogram_loss.py): None, or the arguments of NeuralStyleTransfer.set_histogram_loss, likewise; `remd`
    (remd_loss.py): None, or the arguments of NeuralStyleTransfer.set_relaxed_emd, likewise; `selfsim` (selfsim_loss.py): None, or
    the arguments of NeuralStyleTransfer.set_self_similarity, likewise; `xcorr` (xcorr_loss.py): None, or the arguments of
    NeuralStyleTransfer.set_shifted_gram, likewise."""
    settings = _job.JobSettings(for_job=True, **keywords)

    def level_shapes(img):      # (the level sizes follow from the image size: top level first)
        ih, iw = np.shape(img)[:2]
        return [host_image.level_size(ih, iw, lvl) for lvl in range(max(levels_num - 1, 0), -1, -1)]

    resolved = settings.resolve(lambda: level_shapes(content_n_style.content[1]), lambda: level_shapes(content_n_style.style[1]))
    if patches is not None:
        style_set, use_relu = resolved["taps"][1:] if "taps" in resolved else (_taps.DEFAULT_STYLE_INDICES, True)
        checked = _mrf.normalize_mrf(*patches, style_indices=style_set, use_relu=use_relu, levels_num=max(levels_num, 1))
        _mrf.check_exclusive(checked, regions=resolved.get("regions"), extra_styles=keywords.get("extra_styles"))
        _mrf.check_sizes(checked, level_shapes(content_n_style.content[1]), level_shapes(content_n_style.style[1]))
        patches = patches if checked is not None else None
    if semantics is not None:
        if _mrf.normalize_semantic(*semantics) is None:
            semantics = None
        elif patches is None:
            raise ValueError("semantic_content / semantic_style steer the MRF term: mrf_weight is off")
    if histograms is not None:
        style_set, use_relu = resolved["taps"][1:] if "taps" in resolved else (_taps.DEFAULT_STYLE_INDICES, True)
        checked = _hist.normalize_hist(*histograms, style_indices=style_set, use_relu=use_relu, levels_num=max(levels_num, 1))
        _hist.check_exclusive(checked, regions=resolved.get("regions"), extra_styles=keywords.get("extra_styles"))
        histograms = histograms if checked is not None else None
    if remd is not None:
        style_set, use_relu = resolved["taps"][1:] if "taps" in resolved else (_taps.DEFAULT_STYLE_INDICES, True)
        checked = _remd.normalize_remd(*remd, style_indices=style_set, use_relu=use_relu, levels_num=max(levels_num, 1))
        _remd.check_exclusive(checked, regions=resolved.get("regions"), extra_styles=keywords.get("extra_styles"))
        _remd.level_strides(checked, level_shapes(content_n_style.content[1]), level_shapes(content_n_style.style[1]))
        remd = remd if checked is not None else None
    if selfsim is not None:
        content_i, style_set, use_relu = resolved.get("taps", (_taps.DEFAULT_CONTENT_INDEX, _taps.DEFAULT_STYLE_INDICES, True))
        checked = _selfsim.normalize_selfsim(*selfsim, content_index=content_i, style_indices=style_set, use_relu=use_relu,
                                             levels_num=max(levels_num, 1))
        _selfsim.check_exclusive(checked, regions=resolved.get("regions"), extra_styles=keywords.get("extra_styles"))
        _selfsim.level_strides(checked, level_shapes(content_n_style.content[1]))
        selfsim = selfsim if checked is not None else None
    if xcorr is not None:
        _, style_set, use_relu = resolved.get("taps", (_taps.DEFAULT_CONTENT_INDEX, _taps.DEFAULT_STYLE_INDICES, True))
        checked = _xcorr.normalize_xcorr(*xcorr, style_indices=style_set, use_relu=use_relu, levels_num=max(levels_num, 1))
        _xcorr.check_exclusive(checked, regions=resolved.get("regions"), extra_styles=keywords.get("extra_styles"))
        _xcorr.level_carries(checked, level_shapes(content_n_style.content[1]), level_shapes(content_n_style.style[1]))
        xcorr = xcorr if checked is not None else None
    extra_styles = keywords.get("extra_styles")
    extra_styles = list(extra_styles) if extra_styles is not None else []
    for img in extra_styles:
        if np.ndim(img) != 3 or np.shape(img)[2] != 3:
            raise ValueError(f"extra_styles: expected HWC images with 3 channels, got shape {np.shape(img)}")
    return _transfer(content_n_style, content_weight, style_weight, tv_weight, optimizer, model, init_method, iters_num, levels_num,
                     noise_factor, noise_levels, noise_levels_central_amplitude, noise_levels_peripheral_amplitude,
                     noise_levels_dispersion, device, settings, keywords.get("preserve_color"), extra_styles,
                     keywords.get("style_blend"), start, patches, semantics, histograms, remd, selfsim,
                     **({} if xcorr is None else {"xcorr": xcorr}))        # (by name, and only when set: `selfsim` stays the last positional)


async def _transfer(content_n_style, content_weight, style_weight, tv_weight, optimizer, model, init_method, iters_num, levels_num,
                    noise_factor, noise_levels, noise_levels_central_amplitude, noise_levels_peripheral_amplitude,
                    noise_levels_dispersion, device, settings, preserve_color, extra_styles, style_blend, start=None, patches=None,
                    semantics=None, histograms=None, remd=None, selfsim=None, xcorr=None):
    """neural_style_transfer() below its settings validation: `settings` is its validated JobSettings, `extra_styles` its
    checked list.  `start` (video.py): None, or a callable (setup engine, level-0 (h, w)) -> (start image: a device HWC
    tensor the job starts from in place of the `init_method` image, anchor levels, weight levels, gamma) - the arguments of
    NeuralStyleTransfer.set_anchor - called once the level sizes are known.  `patches` (patch_match.py): None, or the checked
    arguments of NeuralStyleTransfer.set_patch_match; `semantics`: None, or those of NeuralStyleTransfer.set_patch_semantics;
    `histograms` (histogram_loss.py): None, or those of NeuralStyleTransfer.set_histogram_loss; `remd` (remd_loss.py): None,
    or those of NeuralStyleTransfer.set_relaxed_emd; `selfsim` (selfsim_loss.py): None, or those of
    NeuralStyleTransfer.set_self_similarity; `xcorr` (xcorr_loss.py): None, or those of NeuralStyleTransfer.set_shifted_gram."""
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
    anchor = None
    if start is None:
        init_img, tag = device_image.initial_image(
            setup, init_method, content_dev, style_dev, content_levels[0], style_levels[0], level,
            noise_factor, noise_levels, noise_levels_central_amplitude, noise_levels_peripheral_amplitude,
            noise_levels_dispersion, style_init=style_init)
        init_name = {"random": "random", "content": content_n_style.content[0], "style": content_n_style.style[0]}[tag]
    else:
        init_img, *anchor = start(setup, tuple(content_levels[0].shape[:2]))
        init_name = "previous frame"

    nst = NeuralStyleTransfer(device, model, style_levels, optimizer)
    if anchor is not None:
        nst.set_anchor(*anchor)
    if patches is not None:
        nst.set_patch_match(*patches)
    if semantics is not None:
        nst.set_patch_semantics(*semantics)
    if histograms is not None:
        nst.set_histogram_loss(*histograms)
    if remd is not None:
        nst.set_relaxed_emd(*remd)
    if selfsim is not None:
        nst.set_self_similarity(*selfsim)
    if xcorr is not None:
        nst.set_shifted_gram(*xcorr)
    # (the extra styles as their pyramids; "histogram" has recoloured the style levels above)
    settings.update(extra_styles=extra_levels, style_blend=style_blend if extra_levels else None)
    if preserve_color == "histogram":
        settings.update(preserve_color=None)
    nst.settings = settings
    lr_start = 10.0
    async for img, cur_iter in nst.process(content_levels, init_img, lr_start, iters_num, content_weight,
                                           style_weight, tv_weight, init_name):
        yield cur_iter / iters_num * 100.0, img
