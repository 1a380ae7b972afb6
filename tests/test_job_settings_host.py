"""Host: job_settings.SETTINGS is the one list of the optional job settings - its keywords are those of Config and of
neural_style_transfer(), every key it can emit is taken by the real _make_job and consumed, `apply` makes the engine calls of
tests/golden/job_call_transcripts.json (recorded from real device jobs by tools/job_transcript.py) and
StyleEngine.reset_job_settings undoes the settings in the order a pooled engine needs."""
import inspect
import json
import os

import pytest

from artstyletransfer_amd import job_settings

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "job_call_transcripts.json")
TARGET_CALLS = ("set_guidance", "set_targets", "set_targets_blend", "set_targets_guided")


class RecordingEngine:
    """A plain object that logs method name and arguments of whatever is called on it."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        return lambda *args, **kwargs: self.calls.append([name, list(args), kwargs])


def as_json(v):
    return json.loads(json.dumps(v))


def test_the_table_has_the_keywords_of_the_job_driver_and_of_config():
    import neural_style_transfer as nst
    from artstyletransfer_amd import config
    kw_only = [(p.name, p.default) for p in inspect.signature(nst.neural_style_transfer).parameters.values()
               if p.kind is inspect.Parameter.KEYWORD_ONLY]
    assert kw_only == list(job_settings.KEYWORDS.items())
    assert len(kw_only) == 19
    cfg = config.Config()
    for name, default in job_settings.KEYWORDS.items():
        assert getattr(cfg, name) == default and name not in repr(cfg)
    assert config._KW_ONLY == job_settings.KEYWORDS
    assert job_settings.KEYS == ("taps", "color", "pooling", "blend", "style_weights", "regions", "laplacian", "gram_shift",
                                 "matting", "moments")
    # the groups and their leaders
    led = {tuple(s.keywords) for s in job_settings.SETTINGS if s.hand_on == "led"}
    assert led == {("laplacian_weight", "laplacian_pool"), ("matting_weight", "matting_epsilon"),
                   ("moment_weight", "moment_terms", "moment_epsilon")}


def test_every_key_is_taken_by_the_real_job_and_consumed():
    from artstyletransfer_amd import engine
    from artstyletransfer_amd import neural_style_transfer as impl
    assert inspect.signature(impl._make_job).parameters["settings"].kind is inspect.Parameter.VAR_KEYWORD
    assert list(inspect.signature(impl._DeviceJob.__init__).parameters)[-1] == "settings"
    with pytest.raises(TypeError, match="not_a_setting"):       # (refused before a device job is made)
        impl._make_job(None, "adam", [], [], None, 10.0, not_a_setting=1)
    for s in job_settings.SETTINGS:
        if s.key in job_settings.APPLY_ORDER:
            assert callable(getattr(engine.StyleEngine, s.setter))
        else:
            assert s.setter is None and s.key in impl._DeviceJob.CONSUMES
    assert set(job_settings.APPLY_ORDER) <= set(job_settings.KEYS) and len(set(job_settings.APPLY_ORDER)) == 8


@pytest.mark.parametrize("name", ["plain", "taps, avg pooling, style weights", "luminance, laplacian, matting",
                                  "gram shift, moments, blend", "regions"])
def test_apply_makes_the_recorded_engine_calls(name):
    """The calls a real device job made between configure and its first target call are `apply`'s on a fake engine."""
    job = json.load(open(GOLDEN))[name]
    calls = job["calls"]
    assert calls[0][0] == "configure"
    first_target = next(i for i, c in enumerate(calls) if c[0] in TARGET_CALLS)
    recorded = calls[1:first_target]
    assert all(c[0] not in TARGET_CALLS and c[0] != "configure" for c in recorded)
    fake = RecordingEngine()
    # (what apply reads holds numbers and strings only; blend and regions, arrays in the job, are _DeviceJob's)
    job_settings.apply(fake, {k: v for k, v in job["settings"].items() if k in job_settings.APPLY_ORDER})
    assert as_json(fake.calls) == recorded
    order = [job_settings._BY_KEY[k].setter for k in job_settings.APPLY_ORDER]
    assert [c[0] for c in recorded] == [m for m in order if m in {c[0] for c in recorded}]


def test_the_recorded_jobs_use_every_setting():
    jobs = json.load(open(GOLDEN))
    assert set().union(*(set(j["settings"]) for j in jobs.values())) == set(job_settings.KEYS)
    assert jobs["plain"]["settings"] == {} and [c[0] for c in jobs["plain"]["calls"]] == ["configure", "set_targets", "set_targets"]


def test_apply_order_is_the_device_jobs():
    fake = RecordingEngine()
    job_settings.apply(fake, {"color": "luminance", "moments": (1, 2, 3), "gram_shift": (4, 5), "matting": (6, 7),
                              "laplacian": (8, 9), "style_weights": (1,) * 6, "pooling": "avg", "taps": (4, (1,), True),
                              "blend": object(), "regions": object()})
    assert fake.calls == [["set_taps", [4, (1,), True], {}], ["set_pooling", ["avg"], {}], ["set_style_weights", [(1,) * 6], {}],
                          ["set_laplacian", [8, 9], {}], ["set_matting", [6, 7], {}], ["set_gram_shift", [4, 5], {}],
                          ["set_moments", [1, 2, 3], {}], ["set_color", ["luminance"], {}]]


def test_reset_job_settings_makes_the_eight_resets_in_order():
    from artstyletransfer_amd import engine
    fake = RecordingEngine()
    engine.StyleEngine.reset_job_settings(fake)
    assert [c[0] for c in fake.calls] == ["reset_style_weights", "reset_taps", "reset_color", "reset_pooling", "reset_laplacian",
                                          "reset_gram_shift", "reset_matting", "reset_moments"]
    assert all(c[1:] == [[], {}] for c in fake.calls)


def test_configure_clears_the_cached_loss_terms():
    from artstyletransfer_amd import engine
    assert [attr for attr, _, _, cleared in engine._JOB_SETTINGS if cleared] == ["laplacian", "gram_shift", "matting", "moment_loss"]
    assert all(reader is None or callable(getattr(engine.StyleEngine, reader)) for _, reader, _, _ in engine._JOB_SETTINGS)


def test_the_record_resolves_what_the_setters_gave():
    """One record through its three stages: construction validates, update replaces a group, resolve normalises against the
    job (a number of the moment loss goes on the style maps of the taps) and leaves the settings that are off out."""
    s = job_settings.JobSettings(pooling="avg", laplacian_weight=5, matting_weight=0)
    assert s.resolve([(64, 96)], [(64, 96)]) == {"pooling": "avg", "laplacian": ((4,), (5.0,))}
    s.update(content_layer=4, style_layers=[1, 4], use_relu=True)
    s.update(moment_weight=2.0, moment_terms="mean", moment_epsilon=1e-5)
    s.update(laplacian_weight=None, laplacian_pool=4)
    out = s.resolve(lambda: pytest.fail("no setting needs the level sizes"), None)
    zeros = (0.0,) * 6
    assert out == {"pooling": "avg", "taps": (4, (1, 4), True), "moments": ((0.0, 2.0, 0.0, 0.0, 2.0, 0.0), zeros, 1e-5)}
    with pytest.raises(ValueError, match="too small for pool"):
        job_settings.JobSettings(laplacian_weight=1, laplacian_pool=32).resolve([(64, 96), (32, 48)], [])
    with pytest.raises(TypeError):
        job_settings.JobSettings(no_such_keyword=1)
    with pytest.raises(ValueError, match="use_relu"):
        job_settings.JobSettings(for_job=True, use_relu="yes")
    job_settings.JobSettings(use_relu="yes")            # (Config does not look at the taps: the job driver refuses them)


def test_handed_on_follows_the_three_rules():
    from artstyletransfer_amd import config
    assert job_settings.handed_on(config.Config()) == {}
    assert job_settings.handed_on(object()) == {}                  # (a config without the extensions is the reference's)
    cfg = config.Config(use_relu=False, style_blend=[1.0], laplacian_weight=0, moment_terms="std")
    assert job_settings.handed_on(cfg) == {"use_relu": False, "style_blend": [1.0], "laplacian_weight": 0, "laplacian_pool": 4}
