"""Feature network surface of the reference (neural_nets.py:10-68) on top of the HIP engine.

`Vgg19` keeps the reference's attributes (`layer_names`, `content_feature_maps_index`,
`style_feature_maps_indices`) and returns the same `VggOutputs` namedtuple, but holds no
torch modules: the 13 frozen conv layers live, re-laid-out, inside a `StyleEngine` per GPU.
The reference downloads torchvision's pretrained checkpoint into TORCH_HOME = its own directory
(neural_nets.py:19, neural_style_transfer.py:8-10).  Here the file is only ever read from disk:
NST_VGG19_WEIGHTS (a path), else `$TORCH_HOME/hub/checkpoints/vgg19-*.pth`, else the same under the
directory of the drop-in modules and under ~/.cache/torch.  Without a file `load_weights` RAISES - a
switched-over deployment must not silently paint with random weights - unless NST_SYNTHETIC_WEIGHTS=1
opts into the seeded synthetic set (benchmarks, demos without a checkpoint)."""
from __future__ import annotations

import glob
import os
import threading
import warnings
from collections import namedtuple
from typing import Dict, List, Tuple

import torch

from . import synthetic
from .engine import StyleEngine
from .pooling_modes import check_pooling
from .taps import DEFAULT_CONTENT_INDEX, DEFAULT_STYLE_INDICES, LAYER_NAMES

_FEATURE_CONV_INDICES = (0, 2, 5, 7, 10, 12, 14, 16, 19, 21, 23, 25, 28)   # torchvision vgg19.features

_weights_cache = None
_engines: Dict[int, StyleEngine] = {}
_lock = threading.Lock()


def state_dict_to_weights(sd) -> List[Tuple[torch.Tensor, torch.Tensor]]:
    """torchvision vgg19 state dict -> the 13 (weight, bias) pairs conv1_1..conv5_1 (features.0 ... features.28)."""
    ws = []
    for i, (cin, cout) in zip(_FEATURE_CONV_INDICES, synthetic.VGG19_CONV_SHAPES):
        try:
            w, b = sd[f"features.{i}.weight"], sd[f"features.{i}.bias"]
        except KeyError as e:
            raise KeyError(f"not a torchvision vgg19 state dict: {e} is missing") from e
        if tuple(w.shape) != (cout, cin, 3, 3) or tuple(b.shape) != (cout,):
            raise ValueError(f"features.{i}: expected weight {(cout, cin, 3, 3)} and bias {(cout,)}, got "
                             f"{tuple(w.shape)} and {tuple(b.shape)}")
        ws.append((w.detach().float().contiguous(), b.detach().float().contiguous()))
    return ws


def find_checkpoint() -> str | None:
    """The pretrained file where the reference's download would have put it (never fetched here)."""
    explicit = os.environ.get("NST_VGG19_WEIGHTS")
    if explicit:
        return explicit
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))      # directory of the drop-in modules
    homes = [os.environ.get("TORCH_HOME"), root, os.path.join(os.path.expanduser("~"), ".cache", "torch")]
    for home in homes:
        if not home:
            continue
        hits = sorted(glob.glob(os.path.join(home, "hub", "checkpoints", "vgg19-*.pth")))
        if hits:
            return hits[0]
    return None


def load_weights() -> List[Tuple[torch.Tensor, torch.Tensor]]:
    global _weights_cache
    if _weights_cache is not None:
        return _weights_cache
    path = find_checkpoint()
    if path:
        ws = state_dict_to_weights(torch.load(path, map_location="cpu"))
    elif os.environ.get("NST_SYNTHETIC_WEIGHTS") == "1":
        warnings.warn("NST_SYNTHETIC_WEIGHTS=1: using seeded synthetic VGG19 weights "
                      "(results are not artistically meaningful)")
        ws = synthetic.vgg19_weights()
    else:
        raise FileNotFoundError(
            "no VGG19 checkpoint found: set NST_VGG19_WEIGHTS to a torchvision vgg19 state-dict file, or put "
            "vgg19-*.pth under $TORCH_HOME/hub/checkpoints (where the reference's download caches it); "
            "NST_SYNTHETIC_WEIGHTS=1 opts into seeded synthetic weights (benchmarks only)")
    _weights_cache = ws
    return ws


def set_weights(weights) -> None:
    """Install (weight, bias) pairs conv1_1..conv5_1; drops engines built on the old ones."""
    global _weights_cache
    with _lock:
        _weights_cache = list(weights)
        for e in _engines.values():
            e.close()
        _engines.clear()
        for pool in _idle.values():
            for e in pool:
                e.close()
        _idle.clear()


_idle: Dict[int, List[StyleEngine]] = {}       # engines (contexts with the weights uploaded) waiting for their next job, per GPU
_IDLE_MAX = 2                                  # config.simultaneous_tasks_count jobs per GPU is the scheduler's default


def lease_engine(device) -> StyleEngine:
    """An engine for ONE job's targets and workspace (a LossBuilder, a job of the loop).  Contexts are re-used: building
    one means re-laying out and uploading 13 layers of weights (0.25 s, 260 MB), configuring one for the next job only
    re-allocates the pyramid workspace.  Give it back with `return_engine`."""
    dev = torch.device(device)
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    with _lock:
        pool = _idle.get(idx)
        if pool:
            return pool.pop()
    return StyleEngine(load_weights(), idx)


def return_engine(eng: StyleEngine) -> None:
    """Back to the per-GPU pool, with unit style layer weights, the default taps, RGB, max pooling, no Laplacian, matting or moment term and the plain Gram statistic: the
    next job must not inherit this one's."""
    if getattr(eng, "ctx", None) is None:
        return
    idx = eng.device.index
    with _lock:
        pool = _idle.setdefault(idx, [])
        keep = len(pool) < _IDLE_MAX and _weights_cache is not None and getattr(eng, "weights_id", None) == id(_weights_cache)
    if keep:
        try:
            eng.clear_guidance()               # (no region guidance: the re-configuration below drops it with the levels too)
            eng.release_job()                  # the workspace goes back now, only the weights stay resident (and the Laplacian setting goes)
            eng.reset_job_settings()           # (the loss terms are already off: release_job configured the context anew)
        except Exception:
            keep = False
    if keep:
        with _lock:
            _idle.setdefault(idx, []).append(eng)
        return
    eng.close()


def shared_engine(device) -> StyleEngine:
    """The per-GPU engine used by the stand-alone helpers (gram_matrix, Vgg19.forward, ...)."""
    dev = torch.device(device)
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    with _lock:
        if idx not in _engines:
            _engines[idx] = StyleEngine(load_weights(), idx)
        return _engines[idx]


class _Vgg19Call(type):
    """Vgg19(..., pooling="max" | "avg"): the keyword-only extension is taken by the class call, so that Vgg19.__init__
    keeps exactly the reference's parameter list (requires_grad, show_progress, use_relu).  Validated before the
    constructor runs (ValueError)."""

    def __call__(cls, *args, pooling="max", **kwargs):
        check_pooling(pooling)
        net = super().__call__(*args, **kwargs)
        net.pooling = pooling
        return net


class Vgg19(metaclass=_Vgg19Call):
    """Only the layers the original NST paper uses are exposed (relu1_1, relu2_1, relu3_1, relu4_1,
    conv4_2, relu5_1); 'conv4_2' carries ReLU(conv4_2) exactly as the reference's in-place ReLU
    leaves it.  use_relu=False names them conv1_1 ... conv5_1 as the reference does; torchvision's
    in-place ReLUs still leave maps 0..4 post-ReLU there, and only map 5 is conv5_1 BEFORE its ReLU.
    pooling="avg" (extension, keyword-only): every MaxPool2d of the network is an AvgPool2d(2, 2) (Gatys et al. 2016)."""

    def __init__(self, requires_grad=False, show_progress=False, use_relu=True):
        if requires_grad:
            raise NotImplementedError("the feature network is frozen; only the image is optimised")
        self.pooling = "max"                    # Vgg19(..., pooling=): set by the class call
        self.use_relu = bool(use_relu)
        self.layer_names = list(LAYER_NAMES[self.use_relu])
        self.offset = 1 if self.use_relu else 0
        self.content_feature_maps_index = 4
        self.style_feature_maps_indices = [0, 1, 2, 3, 5]
        self.weights = load_weights()
        self.device = None

    def to(self, device):
        self.device = torch.device(device)
        return self

    def eval(self):
        return self

    def parameters(self):
        for w, b in self.weights:
            yield w
            yield b

    def forward(self, x: torch.Tensor):
        if self.use_relu and self.pooling == "max":
            outs = shared_engine(x.device).vgg_features(x.contiguous())
        else:
            # the pre-ReLU conv5_1 and the pooling are settings of the context: a pooled one, handed back with the defaults
            eng = lease_engine(x.device)
            try:
                if not self.use_relu:
                    eng.set_taps(DEFAULT_CONTENT_INDEX, DEFAULT_STYLE_INDICES, use_relu=False)
                eng.set_pooling(self.pooling)
                outs = eng.vgg_features(x.contiguous())
            finally:
                return_engine(eng)
        return namedtuple("VggOutputs", self.layer_names)(*outs)

    __call__ = forward
