"""The long-range style term ("xcorr") as a job: neural_style_transfer() with the cross-correlations of the chosen maps with
spatially shifted copies of themselves held to the style's - Berger & Memisevic, "Incorporating Long-Range Consistency in
CNN-based Texture Generation" (ICLR 2017).  The term is data of one job (nst_level_set_xcorr in include/nst_hip.h has the
definition; xcorr_modes.py the normaliser), so it has a function of its own, as the self-similarity term has: the parameter
lists of the existing functions stay as they are."""
from __future__ import annotations

from . import hist_modes as _hist
from . import laplacian_modes as _lap
from . import matting_modes as _mat
from . import moment_modes as _mom
from . import mrf_modes as _mrf
from . import neural_style_transfer as _nst
from . import remd_modes as _remd
from . import selfsim_loss as _sl
from . import selfsim_modes as _selfsim
from . import xcorr_modes as _xcorr


async def neural_style_transfer_xcorr(content_n_style,
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
                                      semantic_weight=_mrf.DEFAULT_SEMANTIC_WEIGHT,
                                      hist_weight=None, hist_bins=_hist.DEFAULT_BINS, hist_levels=None,
                                      remd_weight=None, remd_samples=_remd.DEFAULT_SAMPLES, remd_epsilon=_remd.DEFAULT_EPSILON,
                                      remd_levels=None,
                                      selfsim_weight=None, selfsim_samples=_selfsim.DEFAULT_SAMPLES,
                                      selfsim_epsilon=_selfsim.DEFAULT_EPSILON, selfsim_levels=None,
                                      xcorr_weight=None, xcorr_shifts=_xcorr.DEFAULT_SHIFTS, xcorr_levels=None):
    """neural_style_transfer_selfsim() - its parameters, in their order, and the same async generator of (percent, image) -
    with the long-range style term: `xcorr_weight`: None or 0 - exactly neural_style_transfer_selfsim() - or a number (that
    weight on those of relu2_1, relu3_1, relu4_1 that are style maps of the job), six numbers by map index of
    Vgg19.layer_names, or a dict {map index or name: number}.  It has no default: the statistic is a Gram matrix, so a weight
    that matters is of the order of `style_weight`.  `xcorr_shifts`: integers k - the axis shifts (k, 0) and (0, k) - or pairs
    (dx, dy), 0..64 in map pixels, at most 16 after expansion, all distinct; the term is the mean over them, so a weight means
    the same whatever the list is.  `xcorr_levels`: None for every level, or the pyramid levels that carry the term, as
    StyleEngine numbers them (0 = the full resolution).  Every level gets the style level image its targets are made from.
    The weights are the term's own: `style_weight` and `style_layer_weights` do not scale it, and it reads the raw map
    whatever `gram_shift` is.
    ValueError before any GPU work, besides neural_style_transfer_selfsim()'s: a malformed setting; a positive weight on a map
    that is not a style map of the job; a shift that is not smaller than a weighted map of a carrying level, of either image;
    the term together with `extra_styles` or with `content_regions` / `style_regions`.  (Stripe sharding refuses the term
    where it is set up: PixelOptimizer.shard_stripes.)"""
    kw = dict(content_layer=content_layer, style_layers=style_layers, use_relu=use_relu, preserve_color=preserve_color,
              pooling=pooling, extra_styles=extra_styles, style_blend=style_blend, style_layer_weights=style_layer_weights,
              content_regions=content_regions, style_regions=style_regions, region_weights=region_weights,
              laplacian_weight=laplacian_weight, laplacian_pool=laplacian_pool, gram_shift=gram_shift, matting_weight=matting_weight,
              matting_epsilon=matting_epsilon, moment_weight=moment_weight, moment_terms=moment_terms, moment_epsilon=moment_epsilon)
    args = (content_n_style, content_weight, style_weight, tv_weight, optimizer, model, init_method, iters_num, levels_num,
            noise_factor, noise_levels, noise_levels_central_amplitude, noise_levels_peripheral_amplitude, noise_levels_dispersion)
    mrf_kw = dict(mrf_weight=mrf_weight, mrf_stride=mrf_stride, mrf_epsilon=mrf_epsilon, mrf_levels=mrf_levels)
    sem_kw = dict(semantic_content=semantic_content, semantic_style=semantic_style, semantic_weight=semantic_weight)
    hist_kw = dict(hist_weight=hist_weight, hist_bins=hist_bins, hist_levels=hist_levels)
    remd_kw = dict(remd_weight=remd_weight, remd_samples=remd_samples, remd_epsilon=remd_epsilon, remd_levels=remd_levels)
    selfsim_kw = dict(selfsim_weight=selfsim_weight, selfsim_samples=selfsim_samples, selfsim_epsilon=selfsim_epsilon,
                      selfsim_levels=selfsim_levels)
    if _xcorr.normalize_xcorr(xcorr_weight, xcorr_shifts, xcorr_levels) is None:
        job = _sl.neural_style_transfer_selfsim(*args, device, **kw, **mrf_kw, **sem_kw, **hist_kw, **remd_kw, **selfsim_kw)
    else:
        semantic = _mrf.normalize_semantic(semantic_content, semantic_style, semantic_weight)
        patches = None if _mrf.normalize_mrf(mrf_weight, mrf_stride, mrf_epsilon, mrf_levels) is None else tuple(mrf_kw.values())
        if patches is None and not (semantic_content is None and semantic_style is None):
            raise ValueError("semantic_content / semantic_style steer the MRF term: mrf_weight is off")
        histograms = None if _hist.normalize_hist(hist_weight, hist_bins, hist_levels) is None else tuple(hist_kw.values())
        remd = None if _remd.normalize_remd(remd_weight, remd_samples, remd_epsilon, remd_levels) is None else tuple(remd_kw.values())
        selfsim = (None if _selfsim.normalize_selfsim(selfsim_weight, selfsim_samples, selfsim_epsilon, selfsim_levels) is None
                   else tuple(selfsim_kw.values()))
        job = _nst._transfer_from(*args, device=device, start=None, patches=patches,
                                  semantics=None if semantic is None else tuple(sem_kw.values()), histograms=histograms, remd=remd,
                                  selfsim=selfsim, xcorr=(xcorr_weight, xcorr_shifts, xcorr_levels), **kw)
    try:
        async for out in job:
            yield out
    finally:
        await job.aclose()
