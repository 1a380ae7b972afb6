"""GPU: the engine calls real device jobs make while they are set up are those recorded in
tests/golden/job_call_transcripts.json (tools/job_transcript.py wrote it; its jobs use every optional setting between them).
The order of these calls fixes the allocation sequence of the context.  No optimiser step is made."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

pytestmark = pytest.mark.gpu


def test_device_jobs_make_the_recorded_engine_calls(vgg_weights):
    from artstyletransfer_amd import neural_nets
    import job_transcript
    neural_nets.set_weights(vgg_weights)
    golden = json.load(open(os.path.join(ROOT, "tests", "golden", "job_call_transcripts.json")))
    live = json.loads(json.dumps(job_transcript.transcripts()))
    assert list(live) == list(golden)
    for name in golden:
        assert live[name]["settings"] == golden[name]["settings"], name
        assert live[name]["calls"] == golden[name]["calls"], name
