"""GPU: the luminance-only job (preserve_color="luminance", nst_job_set_color) sharded by pyramid levels against the same
job unsharded, through tools/check_sharded_opt.py --luminance: the per-closure all-reduce of the one-plane gradient and the
loss rows (PixelOptimizer.shard_levels over torch.distributed, and nst_opt_shard_levels_comm's packed buffer of
H0*W0 + rows floats behind the C ABI).  Asserted by the tool: the same accept / reject sequence, and by levels on up to
two ranks over RCCL bit-identical loss rows (the gloo rehearsal: the first rows to 1e-5 and the pixel checksum to
1e-9, as for RGB)."""
import os
import re
import socket
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "check_sharded_opt.py")


def _env(**extra):
    env = dict(os.environ, NST_SYNTHETIC_WEIGHTS="1", **extra)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    return env


def test_luminance_job_sharded_by_levels_rehearsed_over_gloo_on_one_gpu():
    """Two ranks share cuda:0, the collectives go through torch.distributed over gloo."""
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), TOOL, "levels", "--backend", "gloo", "--share-gpu", "--luminance", "--levels", "3",
           "--steps", "3"]
    out = subprocess.run(cmd, env=_env(MASTER_ADDR="127.0.0.1"), cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "SHARDED == UNSHARDED" in out.stdout and "world 2 levels luminance pixels 1572864" in out.stdout


def test_luminance_job_through_the_c_abi_communicator():
    """nst_opt_shard_levels_comm with a communicator of one rank: every closure all-reduces ONE packed buffer of the
    one-plane gradient (padded to 64 floats) and the loss row - (1024 * 1536 + 4 * 3 + 1) floats at levels_num = 3."""
    out = subprocess.run([sys.executable, TOOL, "levels", "--c-abi-comm", "--luminance", "--levels", "3", "--steps", "3"],
                         env=_env(), cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "SHARDED == UNSHARDED" in out.stdout
    m = re.search(r"comm \(rank, world, calls, bytes\) \(0, 1, (\d+), (\d+)", out.stdout)
    assert m, out.stdout[-2000:]
    calls, nbytes = int(m.group(1)), int(m.group(2))
    assert calls > 0 and nbytes == calls * (1024 * 1536 + 13) * 4, (calls, nbytes)
