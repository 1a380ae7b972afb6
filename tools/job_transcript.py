"""GPU: the engine calls a device job makes while it is set up - every configure, set_* and reset_* of its StyleEngine
(set_targets* and set_guidance among them) as method name plus arguments, tensors and arrays as their shapes - for a handful
of jobs on 64x96 + 32x48 level images that between them use every optional setting (job_settings.SETTINGS).  The order of
these calls fixes the allocation sequence of the context, so a change of the host layers between Config and the engine must
leave this transcript as it is: tests/golden/job_call_transcripts.json is the output of
    python tools/job_transcript.py > tests/golden/job_call_transcripts.json
and tests/test_hip_job_settings.py compares a live transcript with it; tests/test_job_settings_host.py replays the settings
of every job through job_settings.apply on a fake engine.  No optimiser step is made."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import numpy as np
import torch
from artstyletransfer_amd import gram_modes, moment_modes, neural_nets, regions, style_modes, synthetic
from artstyletransfer_amd import neural_style_transfer as impl
from artstyletransfer_amd.taps import DEFAULT_STYLE_INDICES

H, W, NLEV = 64, 96, 2
SHAPES = [(H >> l, W >> l) for l in range(NLEV)]


def levels(seed, shapes=SHAPES):
    return [synthetic.image(h, w, seed + l) for l, (h, w) in enumerate(shapes)]


def jobs():
    """name -> (style levels, content levels, initial image, the resolved settings _make_job takes as keywords)."""
    content, style = levels(1), levels(11)
    init = (0.6 * content[0] + 0.4 * style[0]).astype(np.float32)
    halves = np.zeros((H, W), dtype=np.int64)
    halves[:, W // 2:] = 1                                   # two regions: the left and the right half
    c_stack, s_stack, lam = regions.check_regions(halves, halves, (1.0, 0.5))
    settings = {
        "plain": {},
        "taps, avg pooling, style weights": {
            "taps": (2, (2, 3), True), "pooling": "avg",
            "style_weights": style_modes.check_style_layer_weights({2: 0.5, 3: 2.0}, style_indices=(2, 3))},
        "luminance, laplacian, matting": {"color": "luminance", "laplacian": ((2, 4), (50.0, 20.0)), "matting": (100.0, 1e-7)},
        "gram shift, moments, blend": {
            "gram_shift": gram_modes.normalize_gram_shift({0: "mean", 2: -1.0, 5: "mean"}),
            "moments": moment_modes.normalize_moments(1e3, "both", 1e-5, style_indices=DEFAULT_STYLE_INDICES),
            "blend": ([levels(21, [(48, 80), (24, 40)])], style_modes.check_style_blend((1.0, 0.5), 2))},
        "regions": {"regions": (regions.level_planes(c_stack, SHAPES, DEFAULT_STYLE_INDICES, "content_regions"),
                                regions.level_planes(s_stack, SHAPES, DEFAULT_STYLE_INDICES, "style_regions"), lam)},
    }
    return {name: (style, content, init, kw) for name, kw in settings.items()}


def describe(v):
    """JSON form of an argument: tensors and arrays as their shapes, tuples as lists."""
    if isinstance(v, torch.Tensor):
        return {"tensor": list(v.shape)}
    if isinstance(v, np.ndarray):
        return {"array": list(v.shape)}
    if isinstance(v, dict):
        return {str(k): describe(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [describe(x) for x in v]
    if isinstance(v, (np.integer, np.floating)):
        return v.item()
    return v


class Recorder:
    """Stands where the job's StyleEngine stands and logs the calls named above before it passes them on."""

    def __init__(self, engine, log):
        self._engine, self._log = engine, log

    def __getattr__(self, name):
        attr = getattr(self._engine, name)
        if not callable(attr) or not (name == "configure" or name.startswith(("set_", "reset_"))):
            return attr

        def logged(*args, **kwargs):
            self._log.append([name, describe(args), describe(kwargs)])
            return attr(*args, **kwargs)

        return logged


def with_recorded_engine(log, body):
    """Run body() with every engine that neural_style_transfer leases wrapped in a Recorder (what return_engine does to a
    pooled engine afterwards is not part of a job's transcript)."""
    lease, give_back = impl.lease_engine, impl.return_engine
    impl.lease_engine = lambda device: Recorder(lease(device), log)
    impl.return_engine = lambda eng: give_back(eng._engine if isinstance(eng, Recorder) else eng)
    try:
        return body()
    finally:
        impl.lease_engine, impl.return_engine = lease, give_back


def transcripts(device=None):
    """{job name: {"settings": ..., "calls": [[method, args, kwargs], ...]}} of jobs(), each built by _make_job and closed."""
    dev = torch.device("cuda", 0) if device is None else device
    out = {}
    for name, (style, content, init, kw) in jobs().items():
        log = []
        with_recorded_engine(log, lambda: impl._make_job(dev, "adam", style, content, init, 10.0, **kw).close())
        out[name] = {"settings": describe(kw), "calls": log}
    return out


if __name__ == "__main__":
    neural_nets.set_weights(synthetic.vgg19_weights(bias_std=2.0))
    json.dump(transcripts(), sys.stdout, indent=1)
    print()
