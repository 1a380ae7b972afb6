"""The MRF style term as a job: neural_style_transfer() with every 3x3 patch of the chosen feature maps pulled towards its
nearest neighbour among the style's patches - Li & Wand, "Combining Markov Random Fields and Convolutional Neural Networks
for Image Synthesis" (CVPR 2016).  The term is data of one job (nst_level_set_patches in include/nst_hip.h has the
definition; mrf_modes.py the normaliser), so it has a function of its own, as the long-term video term has:
neural_style_transfer() and its parameter list stay as they are."""
from __future__ import annotations

from . import laplacian_modes as _lap
from . import matting_modes as _mat
from . import moment_modes as _mom
from . import mrf_modes as _mrf
from . import neural_style_transfer as _nst


async def neural_style_transfer_mrf(content_n_style,
                                    content_weight, style_weight, tv_weight,
                                    optimizer, model, init_method,
                                    iters_num, levels_num, noise_factor, noise_levels, noise_levels_central_amplitude,
                                    noise_levels_peripheral_amplitude, noise_levels_dispersion, device=None, *,
                                    content_layer=None, style_layers=None, use_relu=True, preserve_color=None,
                                    pooling="max", extra_styles=None, style_blend=None, style_layer_weights=None,
                                    content_regions=None, style_regions=None, region_weights=None,
                                    laplacian_weight=None, laplacian_pool=_lap.DEFAULT_POOL, gram_shift=None,
                                    matting_weight=None, matting_epsilon=_mat.DEFAULT_EPSILON,
                                    moment_weight=None, moment_terms="both", moment_epsilon=_mom.DEFAULT_EPSILON,
                                    mrf_weight=None, mrf_stride=_mrf.DEFAULT_STRIDE, mrf_epsilon=_mrf.DEFAULT_EPSILON,
                                    mrf_levels=None):
    """neural_style_transfer() - its parameters, in their order, and the same async generator of (percent, image) - with the
    MRF term: `mrf_weight`: None or 0 - exactly neural_style_transfer() - or a number (that weight on those of relu3_1 and
    relu4_1 that are style maps of the job), six numbers by map index of Vgg19.layer_names, or a dict {map index or name:
    number}; `mrf_stride`: the stride of the style patches, an integer 1..8 (the search costs 1 / stride^2 of stride 1's);
    `mrf_epsilon` > 0; `mrf_levels`: None for every level, or the pyramid levels that carry the term, as StyleEngine numbers
    them (0 = the full resolution, levels_num - 1 = the coarsest): the search on relu4_1 of a 1024x1536 level alone is 5.3
    algorithmic TFLOP per closure, so a large job keeps the term on its coarse levels.  Every level gets the style level image
    its targets are made from: the recoloured one under preserve_color="histogram", the matched luminance plane under
    "luminance".
    ValueError before any GPU work, besides neural_style_transfer()'s: a malformed setting; a positive weight on a map that
    is not a style map of the job; the term together with `extra_styles` (the union of dictionaries is a follow-up) or with
    `content_regions` / `style_regions`; a weighted map that pools below 3x3 on a chosen level, on either image.  (Stripe
    sharding refuses the term where it is set up: PixelOptimizer.shard_stripes.)"""
    kw = dict(content_layer=content_layer, style_layers=style_layers, use_relu=use_relu, preserve_color=preserve_color,
              pooling=pooling, extra_styles=extra_styles, style_blend=style_blend, style_layer_weights=style_layer_weights,
              content_regions=content_regions, style_regions=style_regions, region_weights=region_weights,
              laplacian_weight=laplacian_weight, laplacian_pool=laplacian_pool, gram_shift=gram_shift, matting_weight=matting_weight,
              matting_epsilon=matting_epsilon, moment_weight=moment_weight, moment_terms=moment_terms, moment_epsilon=moment_epsilon)
    args = (content_n_style, content_weight, style_weight, tv_weight, optimizer, model, init_method, iters_num, levels_num,
            noise_factor, noise_levels, noise_levels_central_amplitude, noise_levels_peripheral_amplitude, noise_levels_dispersion)
    if _mrf.normalize_mrf(mrf_weight, mrf_stride, mrf_epsilon, mrf_levels) is None:
        job = _nst.neural_style_transfer(*args, device, **kw)
    else:
        job = _nst._transfer_from(*args, device=device, start=None, patches=(mrf_weight, mrf_stride, mrf_epsilon, mrf_levels), **kw)
    try:
        async for out in job:
            yield out
    finally:
        await job.aclose()


async def neural_style_transfer_mrf_semantic(content_n_style,
                                             content_weight, style_weight, tv_weight,
                                             optimizer, model, init_method,
                                             iters_num, levels_num, noise_factor, noise_levels, noise_levels_central_amplitude,
                                             noise_levels_peripheral_amplitude, noise_levels_dispersion, device=None, *,
                                             content_layer=None, style_layers=None, use_relu=True, preserve_color=None,
                                             pooling="max", extra_styles=None, style_blend=None, style_layer_weights=None,
                                             content_regions=None, style_regions=None, region_weights=None,
                                             laplacian_weight=None, laplacian_pool=_lap.DEFAULT_POOL, gram_shift=None,
                                             matting_weight=None, matting_epsilon=_mat.DEFAULT_EPSILON,
                                             moment_weight=None, moment_terms="both", moment_epsilon=_mom.DEFAULT_EPSILON,
                                             mrf_weight=None, mrf_stride=_mrf.DEFAULT_STRIDE, mrf_epsilon=_mrf.DEFAULT_EPSILON,
                                             mrf_levels=None,
                                             semantic_content=None, semantic_style=None,
                                             semantic_weight=_mrf.DEFAULT_SEMANTIC_WEIGHT):
    """neural_style_transfer_mrf() - its parameters, in their order, and the same async generator - with a pair of semantic
    maps that steers the patch search (Champandard, "Semantic Style Transfer and Turning Two-Bit Doodles into Fine Artworks",
    2016: neural-doodle; nst_level_set_patch_guidance in include/nst_hip.h has the definition): a patch of region r of the
    content prefers style patches of region r of the style.  `semantic_content`, `semantic_style`: each an integer label map
    (H,W) with labels 0..R-1 or a float stack (R,H,W) in [0,1], at any resolution (resized, nearest neighbour, to every level
    that carries the term); R <= 4, equal on both sides.  Both None: exactly neural_style_transfer_mrf().
    `semantic_weight`: gamma of T(i,j) = cos(i,j) + gamma <d_i, e_j>, a finite number >= 0 (0: off).  On post-ReLU maps the
    cosines lie in [0,1], so at gamma >= 1 a candidate of the same region always beats one of another region for one-hot
    descriptors; smaller values trade region for feature similarity.  Value and gradient of the term are unchanged: only the
    matches move.
    ValueError before any GPU work, besides neural_style_transfer_mrf()'s: a malformed map or weight; one map without the
    other; mismatched R; semantic maps while `mrf_weight` is off.  `content_regions` / `style_regions` (the guided Gram
    matrices, another mechanism), `extra_styles` and stripe sharding stay refused with the MRF term."""
    kw = dict(content_layer=content_layer, style_layers=style_layers, use_relu=use_relu, preserve_color=preserve_color,
              pooling=pooling, extra_styles=extra_styles, style_blend=style_blend, style_layer_weights=style_layer_weights,
              content_regions=content_regions, style_regions=style_regions, region_weights=region_weights,
              laplacian_weight=laplacian_weight, laplacian_pool=laplacian_pool, gram_shift=gram_shift, matting_weight=matting_weight,
              matting_epsilon=matting_epsilon, moment_weight=moment_weight, moment_terms=moment_terms, moment_epsilon=moment_epsilon)
    args = (content_n_style, content_weight, style_weight, tv_weight, optimizer, model, init_method, iters_num, levels_num,
            noise_factor, noise_levels, noise_levels_central_amplitude, noise_levels_peripheral_amplitude, noise_levels_dispersion)
    mrf_kw = dict(mrf_weight=mrf_weight, mrf_stride=mrf_stride, mrf_epsilon=mrf_epsilon, mrf_levels=mrf_levels)
    semantic = _mrf.normalize_semantic(semantic_content, semantic_style, semantic_weight)
    if semantic_content is None and semantic_style is None:
        job = neural_style_transfer_mrf(*args, device, **kw, **mrf_kw)
    else:
        if _mrf.normalize_mrf(mrf_weight, mrf_stride, mrf_epsilon, mrf_levels) is None:
            raise ValueError("semantic_content / semantic_style steer the MRF term: mrf_weight is off")
        job = _nst._transfer_from(*args, device=device, start=None, patches=(mrf_weight, mrf_stride, mrf_epsilon, mrf_levels),
                                  semantics=None if semantic is None else (semantic_content, semantic_style, semantic_weight), **kw)
    try:
        async for out in job:
            yield out
    finally:
        await job.aclose()
