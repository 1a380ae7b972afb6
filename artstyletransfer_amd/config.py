"""Configuration surface of the reference (config.py:1-31): same names, same defaults."""
from .job_settings import KEYWORDS, JobSettings

# jobs that may run at once PER GPU (the reference runs everything on device 0; here the
# scheduler multiplies this by the number of GPUs of the node). Use 1 when levels_num > 2.
simultaneous_tasks_count = 2

_DEFAULTS = dict(
    content_weight=1e3,            # weight of the content loss
    style_weight=4e5,              # weight of the style loss
    tv_weight=1e2,                 # weight of the total-variation loss
    optimizer="lbfgs",             # 'lbfgs' | 'adam'
    model="vgg19",                 # 'vgg19'
    init_method="content+noise",   # 'random' | 'content+noise' | 'style'
    levels_num=2,                  # pyramid levels (4 for maximum resolution)
    iters_num=500,                 # closure evaluations (1500 for maximum quality)
    noise_factor=0.95,             # strength of the noise blended into the initial image
    noise_levels=(9, 18, 36, -1, 0),                               # spots along the short axis / spot size / 0 = constant
    noise_levels_central_amplitude=(0.30, 0.20, 0.10, 0.20, 0.20),
    noise_levels_peripheral_amplitude=(0.20, 0.30, 0.40, 0.10, 0.00),
    noise_levels_dispersion=(0.20, 0.30, 0.40, 0.60, 0.30),
)
# extension, keyword-only: the feature maps the losses read (neural_style_transfer(..., content_layer=, style_layers=,
# use_relu=)); None = the reference's content 4 / style [0, 1, 2, 3, 5]; colour preservation (preserve_color=); and the
# pooling of the feature network (pooling=); further style images with their blend (extra_styles=, style_blend=) and the
# per-layer style weights (style_layer_weights=); spatial control (content_regions=, style_regions=, region_weights=); and
# the Laplacian loss (laplacian_weight=, laplacian_pool=); the Gram statistic (gram_shift=); and the matting term
# (matting_weight=, matting_epsilon=); and the moment loss (moment_weight=, moment_terms=, moment_epsilon=).
# Not part of the positional order or the repr.
# job_settings.SETTINGS has the table: what each keyword takes is described at NeuralStyleTransfer.set_*.
_KW_ONLY = KEYWORDS


class Config:
    """Settings of one style-transfer job; positional or keyword arguments in the reference's order
    (config.py:5-18): Config(1e3, 4e5, 1e2, 'adam') and Config(optimizer='adam') both work."""

    def __init__(self, *args, **kwargs):
        names = list(_DEFAULTS)
        if len(args) > len(names):
            raise TypeError(f"Config() takes at most {len(names)} positional arguments ({len(args)} given)")
        for name, value in zip(names, args):
            if name in kwargs:
                raise TypeError(f"Config() got multiple values for argument '{name}'")
            kwargs[name] = value
        unknown = set(kwargs) - set(_DEFAULTS) - set(_KW_ONLY)
        if unknown:
            raise TypeError(f"Config() got unexpected keyword argument(s): {sorted(unknown)}")
        for name, default in {**_DEFAULTS, **_KW_ONLY}.items():
            setattr(self, name, kwargs.get(name, default))
        # (against every map: the style set of the job is checked again where the taps are known)
        JobSettings(**{name: getattr(self, name) for name in _KW_ONLY})

    def __repr__(self):
        return "Config(" + ", ".join(f"{k}={getattr(self, k)!r}" for k in _DEFAULTS) + ")"
