"""Host: mrf_modes, hist_modes and remd_modes bind one implementation (map_term_modes) to their own words - a malformed input
draws the same message from all three, the setting's name apart."""
import pytest

from artstyletransfer_amd import hist_modes, mrf_modes, remd_modes

BINDINGS = ((mrf_modes, "mrf"), (hist_modes, "hist"), (remd_modes, "remd"))
STYLE = (0, 1, 2, 3, 5)
# (what, the call on a module m) - every one raises ValueError
MALFORMED = (
    ("a bad type", lambda m: m.normalize_weights("1.0", STYLE)),
    ("a bad entry", lambda m: m.normalize_weights((0.0, True, 0.0, 0.0, 0.0, 0.0), STYLE)),
    ("a wrong length", lambda m: m.normalize_weights((1.0, 2.0, 3.0), STYLE)),
    ("a negative weight", lambda m: m.normalize_weights(-1.0, STYLE)),
    ("a negative weight by map", lambda m: m.normalize_weights({3: -1.0}, STYLE)),
    ("a positive weight off the style set", lambda m: m.normalize_weights((0.0, 0.0, 0.0, 0.0, 2.0, 0.0), STYLE)),
    ("an unknown map", lambda m: m.normalize_weights({"relu9_9": 1.0}, STYLE)),
    ("levels of a bad type", lambda m: m.normalize_levels(1, 2)),
    ("an empty level collection", lambda m: m.normalize_levels((), 2)),
    ("an out-of-range level", lambda m: m.normalize_levels((0, 2), 2)),
    ("extra styles", lambda m: m.check_exclusive(object(), extra_styles=[1])),
    ("regions", lambda m: m.check_exclusive(object(), regions=object())),
    ("stripes", lambda m: m.check_exclusive(object(), stripes=True)),
)


def _message(call, module, prefix):
    with pytest.raises(ValueError) as err:
        call(module)
    text = str(err.value)
    assert prefix + "_" in text, text             # (the message names the module's own setting)
    return text.replace(prefix + "_", "TERM_")


@pytest.mark.parametrize("what,call", MALFORMED, ids=[w for w, _ in MALFORMED])
def test_the_three_bindings_word_a_refusal_alike(what, call):
    texts = [_message(call, module, prefix) for module, prefix in BINDINGS]
    assert texts[0] == texts[1] == texts[2], (what, texts)


def test_no_default_map_in_the_style_set_differs_in_the_maps_named_only():
    """A plain number weighs the term's default maps; with none of them a style map the message names those maps - the one
    sentence that is a term's own - inside the same frame."""
    for module, prefix in BINDINGS:
        style = sorted(set(range(6)) - set(module._WORDS.default_maps))
        with pytest.raises(ValueError) as err:
            module.normalize_weights(1.0, style)
        assert str(err.value) == (f"{prefix}_weight: {module._WORDS.no_default} is a style map of the job {style}; "
                                  f"give the weights by map")
    assert "relu3_1 nor relu4_1 (indices 2 and 3)" in mrf_modes._WORDS.no_default
    assert "relu1_1 nor relu4_1 (indices 0 and 3)" in hist_modes._WORDS.no_default
    assert "relu2_1, relu3_1, relu4_1 (indices 1, 2, 3)" in remd_modes._WORDS.no_default


def test_well_formed_inputs_come_out_alike():
    for module, _ in BINDINGS:
        assert module.normalize_weights(None) == (0.0,) * 6 and module.normalize_weights(0) == (0.0,) * 6
        assert module.normalize_weights({3: 2.0}, STYLE) == (0.0, 0.0, 0.0, 2.0, 0.0, 0.0)
        on = module._WORDS.default_maps
        assert module.normalize_weights(3.0, range(6)) == tuple(3.0 if i in on else 0.0 for i in range(6))
        assert module.normalize_levels(None) is None and module.normalize_levels([1, 0, 1], 2) == (0, 1)
        assert module.check_exclusive(None, regions=object(), stripes=True, extra_styles=[1]) is None
        assert module.MAX_LEVELS == 8
