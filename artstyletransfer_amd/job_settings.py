"""The optional settings of a job - feature maps, colour preservation, pooling, style blend, per-layer style weights,
regions, the Laplacian loss, the Gram shift, the matting term and the moment loss - described once: `SETTINGS` is the table
every layer between Config and the engine reads, `JobSettings` the record that carries them.  Free of torch so that
config.py can validate with it; everything here raises ValueError before any GPU work.  DESIGN.md ("adding a job setting")
lists what a new setting touches."""
from collections import namedtuple

from . import gram_modes as _gram
from . import laplacian_modes as _lap
from . import matting_modes as _mat
from . import moment_modes as _mom
from . import regions as _regions
from . import style_modes as _style
from . import taps as _taps
from .color_modes import check_preserve_color
from .pooling_modes import check_pooling


def _every_map(style):
    return range(_taps.NUM_MAPS) if style is None else style


# What JobSettings keeps of each setting, from its keywords: validated without a job, None when the setting is off.  `style`
# and `names` are the style set and the flavour of the map names to check against, None while the taps are not known.
def _taps_state(style, names, content_layer, style_layers, use_relu):
    content, style_set = _taps.normalize_taps(content_layer, style_layers, use_relu)
    return None if _taps.is_default(content, style_set, use_relu) else (content, style_set, use_relu)


def _pooling_state(style, names, mode):
    return None if check_pooling(mode) == "max" else mode


def _blend_state(style, names, extra_styles, style_blend):
    # (extra styles, blend as given): the blend is normalised where the style set is known
    extra = list(extra_styles) if extra_styles is not None else []
    if extra or style_blend is not None:
        _style.check_style_blend(style_blend, 1 + len(extra), style_indices=() if style is None else style)
    return (extra, style_blend) if extra else None


def _style_weights_state(style, names, weights):
    # (map names of either flavour while the style set is not known)
    w = _style.check_style_layer_weights(weights, style_indices=_every_map(style), use_relu=names if style is not None else None)
    return None if _style.is_unit(w) else w


def _moments_state(style, names, weight, terms, epsilon):
    # as given: a number goes on the style maps of the job, which resolve() knows
    off = _mom.normalize_moments(weight, terms, epsilon, style_indices=_every_map(style), use_relu=names) is None
    return None if off else (weight, terms, epsilon)


# key:      under which the resolved setting reaches _make_job
# keywords: the public keyword names with their defaults (Config's attributes, neural_style_transfer()'s keyword-only
#           parameters), in the order of that signature; the first one leads the group
# hand_on:  when Task hands a keyword of Config on - "differs": it is not the default; "given": it is not None; "led": the
#           leading keyword is not None, and then the whole group
# state:    (style, names, *keyword values) -> what the record keeps
# setter:   the StyleEngine method apply() calls with the resolved value (`star`: with its items), None where _DeviceJob
#           consumes the value itself
Setting = namedtuple("Setting", "key keywords hand_on state setter star")
SETTINGS = (
    Setting("taps", dict(content_layer=None, style_layers=None, use_relu=True), "differs", _taps_state, "set_taps", True),
    Setting("color", dict(preserve_color=None), "differs", lambda style, names, mode: check_preserve_color(mode),
            "set_color", False),
    Setting("pooling", dict(pooling="max"), "differs", _pooling_state, "set_pooling", False),
    Setting("blend", dict(extra_styles=None, style_blend=None), "given", _blend_state, None, False),
    Setting("style_weights", dict(style_layer_weights=None), "given", _style_weights_state, "set_style_weights", False),
    Setting("regions", dict(content_regions=None, style_regions=None, region_weights=None), "given",
            lambda style, names, c, s, w: _regions.check_regions(c, s, w), None, False),
    Setting("laplacian", dict(laplacian_weight=None, laplacian_pool=_lap.DEFAULT_POOL), "led",
            lambda style, names, weight, pool: _lap.normalize_laplacian(weight, pool), "set_laplacian", True),
    Setting("gram_shift", dict(gram_shift=None), "given",
            lambda style, names, value: _gram.normalize_gram_shift(value, names), "set_gram_shift", True),
    Setting("matting", dict(matting_weight=None, matting_epsilon=_mat.DEFAULT_EPSILON), "led",
            lambda style, names, weight, epsilon: _mat.normalize_matting(weight, epsilon), "set_matting", True),
    Setting("moments", dict(moment_weight=None, moment_terms="both", moment_epsilon=_mom.DEFAULT_EPSILON), "led",
            _moments_state, "set_moments", True),
)
KEYWORDS = {k: v for s in SETTINGS for k, v in s.keywords.items()}
KEYS = tuple(s.key for s in SETTINGS)
# the order of apply()'s engine calls: it fixes the allocation sequence of the context
APPLY_ORDER = ("taps", "pooling", "style_weights", "laplacian", "matting", "gram_shift", "moments", "color")
_BY_KEY = {s.key: s for s in SETTINGS}


def handed_on(cfg):
    """The keywords of `cfg` (a Config, or any object with some of its attributes) that a job is started with: every
    group by its hand_on rule, so that a config without extensions starts the reference's job."""
    out = {}
    for s in SETTINGS:
        names = list(s.keywords)
        if s.hand_on == "led":
            if getattr(cfg, names[0], None) is not None:
                out.update({k: getattr(cfg, k, s.keywords[k]) for k in names})
            continue
        for k in names:
            v = getattr(cfg, k, s.keywords[k])
            if (v != s.keywords[k]) if s.hand_on == "differs" else (v is not None):      # (images and arrays: `is not None`)
                out[k] = v
    return out


def apply(engine, resolved):
    """The engine calls of a resolved dict, between configure and the targets of the levels, in APPLY_ORDER."""
    for key in APPLY_ORDER:
        if key in resolved:
            s = _BY_KEY[key]
            if s.star:
                getattr(engine, s.setter)(*resolved[key])
            else:
                getattr(engine, s.setter)(resolved[key])


class JobSettings:
    """The optional settings of one job in three stages: construction and `update` validate what can be validated without
    a job, `resolve` checks them against the job's style set and level sizes and gives the dict of normalised settings
    (keys of SETTINGS, "off" ones absent) that `apply` turns into engine calls."""

    # The order in which construction looks at the settings, so that of two wrong settings each layer goes on refusing the
    # one it always refused first: Config's (for_job False; it does not look at the taps) and neural_style_transfer()'s.
    _ORDER = {False: ("color", "pooling", "style_weights", "blend", "regions", "laplacian", "matting", "gram_shift", "moments"),
              True: ("taps", "color", "pooling", "style_weights", "blend", "regions", "gram_shift", "moments", "laplacian", "matting")}

    def __init__(self, for_job=False, **keywords):
        """`keywords`: any of KEYWORDS, the rest at their defaults.  for_job=False is Config's validation: the taps are
        not looked at, weights are checked against every map, map names may be of either flavour unless `use_relu` says
        which.  for_job=True is neural_style_transfer()'s: the taps first, everything else against their style set and
        flavour.  Both refuse regions together with extra styles, a Gram shift or the moment loss."""
        unknown = set(keywords) - set(KEYWORDS)
        if unknown:
            raise TypeError(f"JobSettings() got unexpected keyword argument(s): {sorted(unknown)}")
        kw = {**KEYWORDS, **keywords}
        self._state = dict.fromkeys(KEYS)
        style, names = None, kw["use_relu"] if for_job or isinstance(kw["use_relu"], bool) else None
        for key in self._ORDER[for_job]:
            self.update(style, names, **{k: kw[k] for k in _BY_KEY[key].keywords})
            if key == "taps":
                style = (self._state["taps"] or (None, _taps.DEFAULT_STYLE_INDICES))[1]
            self.check_exclusive(key)

    def update(self, style=None, names=None, **keywords):
        """Replace the settings whose keywords are given (a group goes together), validated against every map unless
        `style` names the style set, with map names of either flavour unless `names` says which."""
        for s in SETTINGS:
            if any(k in keywords for k in s.keywords):
                self._state[s.key] = s.state(style, names, *[keywords.pop(k) for k in s.keywords])
        if keywords:
            raise TypeError(f"not a job setting: {sorted(keywords)}")

    def __getitem__(self, key):
        return self._state[key]

    def check_exclusive(self, key):
        """Regions go with neither extra styles, nor a Gram shift, nor the moment loss: ValueError for what `key` excludes."""
        st = self._state
        if key == "regions":
            _regions.check_exclusive(st["regions"], st["blend"][0] if st["blend"] is not None else None)
        elif key == "gram_shift":
            _gram.check_exclusive(st["gram_shift"], st["regions"])
        elif key == "moments":
            _mom.check_exclusive(st["moments"], st["regions"])

    def resolve(self, content_shapes, style_shapes, style_levels=None):
        """The settings against one job: `content_shapes`, `style_shapes` are the (h, w) of the pyramid levels, top level
        first - or callables that give them, called only when a setting needs the sizes (a job without such settings
        fails where the reference's does) - and `style_levels` the number of levels an extra style given as levels must
        have (None: they are images).  Returns {key: normalised setting} for the settings that are on."""
        st = self._state
        if any(st[k] is not None for k in ("laplacian", "matting", "regions")):
            content_shapes = content_shapes() if callable(content_shapes) else content_shapes
        style_set, use_relu = st["taps"][1:] if st["taps"] is not None else (_taps.DEFAULT_STYLE_INDICES, True)
        out = {k: st[k] for k in ("taps", "pooling", "laplacian", "matting", "gram_shift") if st[k] is not None}
        if st["color"] == "luminance":          # ("histogram" recolours the style images: no setting of the device job)
            out["color"] = "luminance"
        if st["style_weights"] is not None:
            out["style_weights"] = _style.check_style_layer_weights(st["style_weights"], style_indices=style_set)
        if st["blend"] is not None:
            extra, blend = st["blend"]
            for lv in extra if style_levels is not None else ():
                if len(lv) != style_levels:
                    raise ValueError(f"an extra style has {len(lv)} levels, the job has {style_levels}")
            out["blend"] = (extra, _style.check_style_blend(blend, 1 + len(extra), style_indices=style_set))
        if st["laplacian"] is not None and len(content_shapes):
            _lap.check_levels(st["laplacian"][0], len(content_shapes), *content_shapes[0])
        if st["matting"] is not None and len(content_shapes):
            _mat.check_levels(len(content_shapes), *content_shapes[0])
        self.check_exclusive("gram_shift")
        if st["moments"] is not None:
            out["moments"] = _mom.normalize_moments(*st["moments"], style_indices=style_set, use_relu=use_relu)
            self.check_exclusive("moments")
        if st["regions"] is not None:
            # resized to every level of the content and of the style pyramid and checked for their masses, on the host
            self.check_exclusive("regions")
            c_stack, s_stack, lam = st["regions"]
            style_shapes = style_shapes() if callable(style_shapes) else style_shapes
            out["regions"] = (_regions.level_planes(c_stack, content_shapes, style_set, "content_regions"),
                              _regions.level_planes(s_stack, style_shapes, style_set, "style_regions"), lam)
        return out
