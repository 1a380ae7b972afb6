"""A sequence of frames stylised with temporal consistency, after Ruder, Dosovitskiy & Brox, "Artistic Style Transfer for
Videos" (GCPR 2016): frame 0 is the plain job; frame i > 0 starts from the previous result warped along the backward optical
flow and is held to it by a per-pixel weighted pixel-space term whose weight is 0 where the flow is unreliable
(nst_level_set_anchor, nst_warp_bilinear and nst_flow_weights in include/nst_hip.h have the definitions).  The flows are
the caller's, from whatever estimator they trust - or, when none are given, estimated on the device between the luminance
planes of consecutive frames by multi-scale Horn-Schunck with warping (nst_flow_estimate; flow_modes.FlowParams): a
baseline that makes the path usable with this project alone, not a replacement for a better estimator - or, handed a
flow_modes.TVL1Params, by TV-L1 on the same pyramid (nst_flow_tvl1_estimate), whose flows stay sharp at motion boundaries.
neural_style_transfer_video_long_term adds the paper's long-term term (section 4.3, eq. 9-10): where the flow to frame i - 1 is
unreliable the frame is held to frame i - 2, then i - 4, ... - whichever offsets are asked for - so what a moving object
uncovers comes back with the texture it had.  The warped earlier results are folded into the ONE anchor and weight plane a
level holds (nst_anchor_fold has the identity that makes this exact); the closure does not change.

The anchor is data of one job, like its content levels - not one of job_settings.SETTINGS: it reaches the job through
NeuralStyleTransfer.set_anchor once the job exists.  Everything here raises ValueError before any GPU work."""
from __future__ import annotations

import numpy as np
import torch

from . import flow_modes as _flow
from . import host_image
from . import job_settings as _job
from . import neural_style_transfer as _nst

__all__ = ["neural_style_transfer_video", "neural_style_transfer_video_long_term", "long_term_anchor", "result_size"]

MAX_LONG_TERM = 7          # offsets besides 1: NST_MAX_ANCHOR_SOURCES sources in one fold


def result_size(frame_shape, levels_num):
    """(h, w) of the images a job of `levels_num` levels yields for a frame of this shape: the size the flows, the weights
    and the warped start image have."""
    return host_image.level_size(int(frame_shape[0]), int(frame_shape[1]), max(int(levels_num) - 1, 0))


def _check_planes(what, seq, count, shape, lo=None, hi=None, per="one per frame after the first"):
    """`seq`: `count` arrays of `shape`, finite (flows may hold non-finite entries: the warp marks them invalid) and - with
    bounds - inside them.  Returns them as contiguous float32 arrays."""
    seq = list(seq)
    if len(seq) != count:
        raise ValueError(f"{what}: expected {count} entries ({per}), got {len(seq)}")
    out = []
    for k, a in enumerate(seq):
        a = np.asarray(a)
        if tuple(a.shape) != tuple(shape):
            raise ValueError(f"{what}[{k}]: expected shape {tuple(shape)} (the size of the yielded images), got {tuple(a.shape)}")
        a = np.ascontiguousarray(a, dtype=np.float32)
        if lo is not None and not (np.isfinite(a).all() and a.min() >= lo and a.max() <= hi):
            raise ValueError(f"{what}[{k}]: values must lie in [{lo}, {hi}]")
        out.append(a)
    return out


def level_anchors(engine, warped_hwc, levels, luminance=False):
    """The anchors of the pyramid levels, top level first, from the warped previous result (a device (h,w,3) tensor): the
    prepared image - under the luminance colour mode the plane StyleEngine.luminance gives, the call that forms the content's
    plane - and StyleEngine.bicubic_half of it level by level: the closure's own down-sampling, so an image that equals the
    anchor has tmp = 0 on every level."""
    top = engine.luminance(warped_hwc) if luminance else engine.prepare_img(warped_hwc)
    out = [top]
    for _ in range(1, levels):
        out.append(engine.bicubic_half(out[-1]))
    return out


def level_weights(plane, levels):
    """The weight planes of the pyramid levels, top level first, from the (h,w) plane of the top level: the 2x2 mean level by
    level, a leftover row or column dropped."""
    out = [plane.contiguous()]
    for _ in range(1, levels):
        out.append(torch.nn.functional.avg_pool2d(out[-1][None, None], 2)[0, 0].contiguous())
    return out


def _planar(flow_hw2, device):
    """(h,w,2) host array -> device (2,h,w): plane 0 = dx, plane 1 = dy."""
    return torch.from_numpy(flow_hw2).to(device).permute(2, 0, 1).contiguous()


def _luminance_plane(setup, frame, h, w):
    """The (h,w) device plane 255 Y of a host frame at the size of the yielded images: what the flows are estimated between."""
    img = torch.from_numpy(np.ascontiguousarray(frame, dtype=np.float32)).to(setup.device)
    return setup.luminance(setup.resize(img, h, w)).reshape(h, w)


def normalize_long_term(long_term):
    """None, or the offsets besides 1 as an ascending tuple of ints: distinct integers >= 2, at most MAX_LONG_TERM."""
    if long_term is None:
        return None
    out = []
    for o in long_term:
        if isinstance(o, (bool, np.bool_)) or not isinstance(o, (int, np.integer)):
            raise ValueError(f"long_term: offsets are integers, got {o!r}")
        if o < 2:
            raise ValueError(f"long_term: offsets are >= 2 (offset 1 is always present), got {int(o)}")
        out.append(int(o))
    if len(set(out)) != len(out):
        raise ValueError(f"long_term: offsets must be distinct, got {tuple(out)}")
    if len(out) > MAX_LONG_TERM:
        raise ValueError(f"long_term: at most {MAX_LONG_TERM} offsets, got {len(out)}")
    return tuple(sorted(out))


def long_term_anchor(engine, results_chw, backward, forward=None, weights=None):
    """(omega, c, parts) of J earlier results, nearest first: results_chw[j] (device (C,h,w)) is warped along backward[j]
    (device (2,h,w), from this frame to that one) and counts under weights[j] if given (device (h,w)), else
    StyleEngine.flow_weights(forward[j], backward[j]) if that forward flow is given, else the warp's valid plane; the warped
    results are folded (StyleEngine.anchor_fold) into the anchor omega (C,h,w) and the weight plane c (h,w), parts (J,h,w)
    being what each source counts with.  `forward`, `weights`: None or J entries, each of which may be None."""
    n = len(results_chw)
    if len(backward) != n or any(x is not None and len(x) != n for x in (forward, weights)):
        raise ValueError(f"long_term_anchor: {n} results need {n} backward flows (and forward flows and weights, where given)")
    sources, planes = [], []
    for j in range(n):
        warped, valid = engine.warp_bilinear(results_chw[j], backward[j])
        if weights is not None and weights[j] is not None:
            c = weights[j]
        elif forward is not None and forward[j] is not None:
            c = engine.flow_weights(forward[j], backward[j])
        else:
            c = valid
        sources.append(warped)
        planes.append(c)
    return engine.anchor_fold(sources, planes, want_parts=True)


async def neural_style_transfer_video(frames, style, backward_flows=None, forward_flows=None, weights=None, *, temporal_weight, cfg,
                                      device=None):
    """Async generator of (frame index, percent, HWC float32 image) over the frames of a sequence, one job per frame in
    order.  `frames`: HWC float [0,1] images of one size; `style`: the style image; `cfg`: a Config - its reference fields
    and the job settings job_settings.handed_on(cfg) gives are used exactly as Task uses them.
    Frame 0 is neural_style_transfer() of (frames[0], style).  Frame i > 0 starts from omega, the last image of frame i - 1
    warped by backward_flows[i-1] - an (h,w,2) array (dx, dy) in pixels from frame i to frame i - 1, at the size of the
    yielded images (result_size); backward_flows None, a flow_modes.FlowParams or a flow_modes.TVL1Params: estimated on the
    device (StyleEngine.flow_estimate: Horn-Schunck with the defaults or these parameters, or - a TVL1Params - TV-L1, which
    keeps the flow sharp around moving objects) from the luminance plane of frame i to that of frame
    i - 1, both resized to the yielded size - and its every level carries the anchor made from omega with weight `temporal_weight`
    (no default: its useful magnitude is a matter of the content, style and TV weights; DESIGN.md 4.12 has measurements) under
    the weight plane c = weights[i-1] if given ((h,w) in [0,1]), else StyleEngine.flow_weights(forward_flows[i-1],
    backward_flows[i-1]) if forward flows are given, else the warp's valid plane.  With estimated backward flows and no
    weights the forward flow is estimated too and c = flow_weights of the pair.  temporal_weight = 0: the warped start
    only.  ValueError before any GPU work for frames of differing sizes, a flow or weight list of the wrong length or shape,
    weights outside [0,1], a negative or non-finite temporal_weight, bad flow parameters, and forward_flows beside
    estimated backward flows (the pair would come from two estimators).  (A job of this driver is never stripe-sharded;
    PixelOptimizer.shard_stripes refuses an engine that carries an anchor.)"""
    job = neural_style_transfer_video_long_term(frames, style, backward_flows, forward_flows, weights, temporal_weight=temporal_weight,
                                                cfg=cfg, device=device)
    try:
        async for item in job:
            yield item
    finally:
        await job.aclose()


async def neural_style_transfer_video_long_term(frames, style, backward_flows=None, forward_flows=None, weights=None, *, temporal_weight,
                                                cfg, device=None, long_term=None, long_term_flows=None):
    """neural_style_transfer_video with the long-term term of Ruder et al. (section 4.3): its arguments, and
    `long_term`: None - exactly neural_style_transfer_video - or the frame offsets besides 1 a frame is also held to: distinct
    integers >= 2, at most 7, in any order.  Frame i uses the offsets j <= i.  Its anchor takes every pixel from frame i - 1
    where c_1 says that flow is reliable, elsewhere from the nearest offset whose c_j does (StyleEngine.anchor_fold; include/
    nst_hip.h, nst_anchor_fold); the start image is that anchor, which keeps the offset-1 warp where no offset is reliable.
    Estimated backward flows (None, a FlowParams, a TVL1Params): for every offset in use the backward flow
    flow_estimate(plane(i), plane(i-j)), the forward flow flow_estimate(plane(i-j), plane(i)), c_j = flow_weights of the
    pair, source j = the last image of frame i - j warped along the backward flow - all on the device; the luminance planes
    and last images of the max(long_term) latest frames are kept, no more.
    Caller flows: `long_term_flows`, a dict offset -> (backward, forward, weights) under the rules of the offset-1 arguments:
    each list has len(frames) - j entries, entry k relating frame k + j to frame k; forward and weights may be None, and c_j
    then falls back as for offset 1.  Its keys are the offsets of `long_term`.
    ValueError before any GPU work, besides neural_style_transfer_video's: an offset < 2, duplicate or non-integer offsets,
    more than 7; long_term_flows without long_term or with other keys; lists of the wrong length or shape; weights outside
    [0,1]; long_term_flows beside estimated backward flows; long_term beside caller backward flows without long_term_flows."""
    frames = list(frames)
    if not frames:
        raise ValueError("frames: at least one frame")
    shape = tuple(np.shape(frames[0]))
    if len(shape) != 3 or shape[2] != 3:
        raise ValueError(f"frames: expected HWC images with 3 channels, got shape {shape}")
    for k, f in enumerate(frames):
        if tuple(np.shape(f)) != shape:
            raise ValueError(f"frames[{k}] has shape {tuple(np.shape(f))}, frames[0] {shape}: the frames of a sequence have one size")
    gamma = float(temporal_weight)
    if not np.isfinite(gamma) or gamma < 0.0:
        raise ValueError(f"temporal_weight must be finite and >= 0, got {temporal_weight!r}")
    n = len(frames) - 1
    h, w = result_size(shape, cfg.levels_num)
    tvl1 = isinstance(backward_flows, _flow.TVL1Params)
    estimate = backward_flows is None or tvl1 or isinstance(backward_flows, _flow.FlowParams)
    if estimate:
        params = _flow.normalize_tvl1(backward_flows) if tvl1 else _flow.normalize_flow(backward_flows)
        if forward_flows is not None:
            raise ValueError("forward_flows cannot be combined with estimated backward flows: give both, or neither")
    bwd = None if estimate else _check_planes("backward_flows", backward_flows, n, (h, w, 2))
    fwd = _check_planes("forward_flows", forward_flows, n, (h, w, 2)) if forward_flows is not None else None
    wts = _check_planes("weights", weights, n, (h, w), 0.0, 1.0) if weights is not None else None
    offsets = normalize_long_term(long_term)
    far = None              # offset -> (backward, forward or None, weights or None): the caller's flows of the offsets >= 2
    if long_term_flows is not None:
        if offsets is None:
            raise ValueError("long_term_flows without long_term: name the offsets")
        if estimate:
            raise ValueError("long_term_flows cannot be combined with estimated backward flows: give the flows of every offset, or none")
        try:
            keys = normalize_long_term(list(long_term_flows))
        except ValueError as e:
            raise ValueError(f"long_term_flows: its keys must be the offsets of long_term {offsets} ({e})") from None
        if keys != offsets:
            raise ValueError(f"long_term_flows: its keys must be the offsets of long_term {offsets}, got {keys}")
        far = {}
        for j in offsets:
            entry = tuple(long_term_flows[j])
            if len(entry) != 3:
                raise ValueError(f"long_term_flows[{j}]: expected (backward, forward, weights), got {len(entry)} entries")
            m, per = max(len(frames) - j, 0), f"one per frame from frame {j} on"
            if entry[0] is None:
                raise ValueError(f"long_term_flows[{j}]: the backward flows are missing")
            far[j] = (_check_planes(f"long_term_flows[{j}] backward", entry[0], m, (h, w, 2), per=per),
                      _check_planes(f"long_term_flows[{j}] forward", entry[1], m, (h, w, 2), per=per) if entry[1] is not None else None,
                      _check_planes(f"long_term_flows[{j}] weights", entry[2], m, (h, w), 0.0, 1.0, per=per) if entry[2] is not None else None)
    elif offsets is not None and not estimate:
        raise ValueError("long_term beside caller backward flows needs long_term_flows: the flows of the other offsets")
    extensions = _job.handed_on(cfg)
    luminance = extensions.get("preserve_color") == "luminance"
    levels = int(cfg.levels_num)
    previous = None

    planes = {}       # frame index -> its luminance plane: frame i's is formed once and read again for frame i + 1

    def plane(setup, j):
        if j not in planes or planes[j].device != setup.device:
            planes[j] = _luminance_plane(setup, frames[j], h, w)
        return planes[j]

    reach = max(offsets, default=1) if offsets is not None else 1
    results = {}      # long_term only: frame index -> its last image, of the `reach` latest frames

    def long_start(i):
        """The start callable of frame i under long_term: the offsets whose frame has a result, nearest first."""
        use = [1] + [j for j in offsets if i - j in results]
        held = [results[i - j] for j in use]

        def start(setup, top_shape):
            if tuple(top_shape) != (h, w) or any(tuple(r.shape[:2]) != (h, w) for r in held):
                raise ValueError(f"the job's top level is {tuple(top_shape)}, the flows are {(h, w)}")
            dev = setup.device
            srcs, back, forw, cs = [], [], [], []
            for j, img in zip(use, held):
                k = i - j           # entry k of an offset's lists relates frame k + j to frame k
                srcs.append(torch.from_numpy(np.ascontiguousarray(img, dtype=np.float32)).to(dev).permute(2, 0, 1).contiguous())
                given = wts if j == 1 else far[j][2] if far is not None else None
                forward = None
                if estimate:
                    here, there = plane(setup, i), plane(setup, k)
                    flow = setup.flow_estimate(here, there, params)
                    if given is None:
                        forward = setup.flow_estimate(there, here, params)
                else:
                    flows, forwards = (bwd, fwd) if j == 1 else far[j][:2]
                    flow = _planar(flows[k], dev)
                    if forwards is not None and given is None:
                        forward = _planar(forwards[k], dev)
                back.append(flow)
                forw.append(forward)
                cs.append(torch.from_numpy(given[k]).to(dev) if given is not None else None)
            for old in [f for f in planes if f <= i - reach]:       # frame i + 1 reads the planes i + 1 - reach .. i + 1
                del planes[old]
            omega, c, _ = long_term_anchor(setup, srcs, back, forw, cs)
            omega = omega.permute(1, 2, 0).contiguous()
            return omega, level_anchors(setup, omega, levels, luminance), level_weights(c, levels), gamma

        return start

    for i, frame in enumerate(frames):
        start = None
        if i > 0 and previous is not None:      # (a job of no iterations yields nothing to warp: the plain job then)
            prev, k = previous, i - 1

            def start(setup, top_shape, prev=prev, k=k):
                if tuple(top_shape) != (h, w) or tuple(prev.shape[:2]) != (h, w):
                    raise ValueError(f"the job's top level is {tuple(top_shape)}, the flows are {(h, w)}")
                dev = setup.device
                src = torch.from_numpy(np.ascontiguousarray(prev, dtype=np.float32)).to(dev).permute(2, 0, 1).contiguous()
                forward = None      # (only the weight plane reads it)
                if estimate:        # backward: frame i -> frame i - 1; forward: the other way
                    here, there = plane(setup, k + 1), plane(setup, k)
                    planes.pop(k, None)
                    flow = setup.flow_estimate(here, there, params)
                    if wts is None:
                        forward = setup.flow_estimate(there, here, params)
                else:
                    flow = _planar(bwd[k], dev)
                    if fwd is not None and wts is None:
                        forward = _planar(fwd[k], dev)
                warped, valid = setup.warp_bilinear(src, flow)
                omega = warped.permute(1, 2, 0).contiguous()
                if wts is not None:
                    c = torch.from_numpy(wts[k]).to(dev)
                elif forward is not None:
                    c = setup.flow_weights(forward, flow)
                else:
                    c = valid
                return omega, level_anchors(setup, omega, levels, luminance), level_weights(c, levels), gamma

            if offsets is not None:
                start = long_start(i)

        job = _frame_job(frame, style, cfg, device, extensions, start)
        last = None
        try:
            async for percent, img in job:
                last = img
                yield i, percent, img
        finally:
            await job.aclose()
        previous = last
        if offsets is not None:
            if last is not None:
                results[i] = last
            results.pop(i - reach, None)


def _frame_job(frame, style, cfg, device, extensions, start):
    """neural_style_transfer() of one frame as Task starts it; `start`: the warped start image and the anchors, frame > 0."""
    pair = _nst.ContentStylePair(("frame", frame), ("style", style))
    args = (pair, cfg.content_weight, cfg.style_weight, cfg.tv_weight, cfg.optimizer, cfg.model, cfg.init_method,
            cfg.iters_num, cfg.levels_num, cfg.noise_factor, cfg.noise_levels, cfg.noise_levels_central_amplitude,
            cfg.noise_levels_peripheral_amplitude, cfg.noise_levels_dispersion)
    if start is None:
        return _nst.neural_style_transfer(*args, device=device, **extensions)
    return _nst._transfer_from(*args, device=device, start=start, **extensions)
