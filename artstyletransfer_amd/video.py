"""A sequence of frames stylised with temporal consistency, after Ruder, Dosovitskiy & Brox, "Artistic Style Transfer for
Videos" (GCPR 2016): frame 0 is the plain job; frame i > 0 starts from the previous result warped along the backward optical
flow and is held to it by a per-pixel weighted pixel-space term whose weight is 0 where the flow is unreliable
(nst_level_set_anchor, nst_warp_bilinear and nst_flow_weights in include/nst_hip.h have the definitions).  The flows are
the caller's, from whatever estimator they trust - or, when none are given, estimated on the device between the luminance
planes of consecutive frames by multi-scale Horn-Schunck with warping (nst_flow_estimate; flow_modes.FlowParams): a
baseline that makes the path usable with this project alone, not a replacement for a better estimator - or, handed a
flow_modes.TVL1Params, by TV-L1 on the same pyramid (nst_flow_tvl1_estimate), whose flows stay sharp at motion boundaries.

The anchor is data of one job, like its content levels - not one of job_settings.SETTINGS: it reaches the job through
NeuralStyleTransfer.set_anchor once the job exists.  Everything here raises ValueError before any GPU work."""
from __future__ import annotations

import numpy as np
import torch

from . import flow_modes as _flow
from . import host_image
from . import job_settings as _job
from . import neural_style_transfer as _nst

__all__ = ["neural_style_transfer_video", "result_size"]


def result_size(frame_shape, levels_num):
    """(h, w) of the images a job of `levels_num` levels yields for a frame of this shape: the size the flows, the weights
    and the warped start image have."""
    return host_image.level_size(int(frame_shape[0]), int(frame_shape[1]), max(int(levels_num) - 1, 0))


def _check_planes(what, seq, count, shape, lo=None, hi=None):
    """`seq`: `count` arrays of `shape`, finite (flows may hold non-finite entries: the warp marks them invalid) and - with
    bounds - inside them.  Returns them as contiguous float32 arrays."""
    seq = list(seq)
    if len(seq) != count:
        raise ValueError(f"{what}: expected {count} entries (one per frame after the first), got {len(seq)}")
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
    extensions = _job.handed_on(cfg)
    luminance = extensions.get("preserve_color") == "luminance"
    levels = int(cfg.levels_num)
    previous = None

    planes = {}       # frame index -> its luminance plane: frame i's is formed once and read again for frame i + 1

    def plane(setup, j):
        if j not in planes or planes[j].device != setup.device:
            planes[j] = _luminance_plane(setup, frames[j], h, w)
        return planes[j]

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

        job = _frame_job(frame, style, cfg, device, extensions, start)
        last = None
        try:
            async for percent, img in job:
                last = img
                yield i, percent, img
        finally:
            await job.aclose()
        previous = last


def _frame_job(frame, style, cfg, device, extensions, start):
    """neural_style_transfer() of one frame as Task starts it; `start`: the warped start image and the anchors, frame > 0."""
    pair = _nst.ContentStylePair(("frame", frame), ("style", style))
    args = (pair, cfg.content_weight, cfg.style_weight, cfg.tv_weight, cfg.optimizer, cfg.model, cfg.init_method,
            cfg.iters_num, cfg.levels_num, cfg.noise_factor, cfg.noise_levels, cfg.noise_levels_central_amplitude,
            cfg.noise_levels_peripheral_amplitude, cfg.noise_levels_dispersion)
    if start is None:
        return _nst.neural_style_transfer(*args, device=device, **extensions)
    return _nst._transfer_from(*args, device=device, start=start, **extensions)
