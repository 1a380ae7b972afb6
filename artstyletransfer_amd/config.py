"""Configuration surface of the reference (config.py:1-31): same names, same defaults."""
from .color_modes import check_preserve_color
from .pooling_modes import check_pooling
from .style_modes import check_style_blend, check_style_layer_weights
from .regions import check_exclusive, check_regions
from .laplacian_modes import DEFAULT_POOL, normalize_laplacian
from .gram_modes import check_exclusive as check_gram_exclusive, normalize_gram_shift
from .matting_modes import DEFAULT_EPSILON, normalize_matting
from .moment_modes import DEFAULT_EPSILON as MOMENT_EPSILON, check_exclusive as check_moment_exclusive, normalize_moments

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
_KW_ONLY = dict(
    content_layer=None,            # index 0..5 or a name of Vgg19.layer_names
    style_layers=None,             # indices / names
    use_relu=True,                 # False: the reference's Vgg19(use_relu=False) taps
    preserve_color=None,           # None | 'luminance' | 'histogram': keep the content's colours (Gatys et al. 2016)
    pooling="max",                 # 'max' | 'avg': average instead of max pooling in VGG19 (Gatys et al. 2016, section 2)
    extra_styles=None,             # further style images (HWC float [0,1]) blended with the pair's style image
    style_blend=None,              # K numbers or a K x 6 array: weight of style k (on map i); K = 1 + len(extra_styles)
    style_layer_weights=None,      # 6 numbers or {map index or name: weight}: the w_l of Gatys et al. 2016
    content_regions=None,          # integer label map (H,W) or float stack (R,H,W) in [0,1] over the content image (Gatys et al. 2017)
    style_regions=None,            # the same over the style image: region r of the content takes its style from region r here
    region_weights=None,           # R numbers >= 0: the lambda_r of the regions' terms (None: ones)
    laplacian_weight=None,         # number or up to 4 numbers >= 0: the gamma_k of the Laplacian loss (Li et al. 2017); None / 0: off
    laplacian_pool=DEFAULT_POOL,   # integer 1..32 or up to 4 distinct ones: the pool sizes p_k of its entries
    gram_shift=None,               # None / 0 | number | 'mean' | 6 entries | {map index or name: number or 'mean'}: shifted / centred Gram matrices
    matting_weight=None,           # number >= 0: the gamma of the matting term (Luan et al. 2017: the photorealism regulariser); None / 0: off
    matting_epsilon=DEFAULT_EPSILON,   # number > 0: the epsilon of the matting Laplacian
    moment_weight=None,            # None / 0 | number | 6 numbers | {map index or name: number}: the moment loss (Li et al. 2017; Huang & Belongie 2017)
    moment_terms="both",           # 'both' | 'mean' | 'std': which of the channel means and deviations are matched
    moment_epsilon=MOMENT_EPSILON, # number > 0: sigma = sqrt(var + epsilon)
)


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
        check_preserve_color(self.preserve_color)
        check_pooling(self.pooling)
        # (against every map: the style set of the job is checked again where the taps are known)
        check_style_layer_weights(self.style_layer_weights, style_indices=range(6))
        if self.extra_styles is not None or self.style_blend is not None:
            check_style_blend(self.style_blend, 1 + len(self.extra_styles or ()), style_indices=())
        check_exclusive(check_regions(self.content_regions, self.style_regions, self.region_weights), self.extra_styles)
        normalize_laplacian(self.laplacian_weight, self.laplacian_pool)
        normalize_matting(self.matting_weight, self.matting_epsilon)
        check_gram_exclusive(normalize_gram_shift(self.gram_shift, self.use_relu if isinstance(self.use_relu, bool) else None),
                             regions=check_regions(self.content_regions, self.style_regions, self.region_weights))
        # (against every map: the style set of the job is checked again where the taps are known)
        check_moment_exclusive(normalize_moments(self.moment_weight, self.moment_terms, self.moment_epsilon, style_indices=range(6),
                                                 use_relu=self.use_relu if isinstance(self.use_relu, bool) else None),
                               regions=check_regions(self.content_regions, self.style_regions, self.region_weights))

    def __repr__(self):
        return "Config(" + ", ".join(f"{k}={getattr(self, k)!r}" for k in _DEFAULTS) + ")"
