"""The preserve_color choices of the job API (Gatys, Bethge, Hertzmann & Shechtman, "Preserving Color in Neural Artistic
Style Transfer", 2016), kept free of torch so that config.py can validate with them."""

PRESERVE_COLOR_MODES = (None, "luminance", "histogram")


def check_preserve_color(mode):
    """ValueError unless `mode` is None, 'luminance' or 'histogram'; returns it."""
    if not (mode is None or (isinstance(mode, str) and mode in PRESERVE_COLOR_MODES)):
        raise ValueError(f"preserve_color must be None, 'luminance' or 'histogram', not {mode!r}")
    return mode
