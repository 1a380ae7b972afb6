"""The pooling choices of the VGG19 feature network (Gatys, Ecker & Bethge, "Image Style Transfer Using Convolutional
Neural Networks", 2016, section 2: average instead of max pooling), kept free of torch so that config.py can validate
with them."""

POOLING_MODES = ("max", "avg")


def check_pooling(mode):
    """ValueError unless `mode` is 'max' or 'avg'; returns it."""
    if not (isinstance(mode, str) and mode in POOLING_MODES):
        raise ValueError(f"pooling must be 'max' or 'avg', not {mode!r}")
    return mode
