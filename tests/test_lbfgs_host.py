"""The host scalars of the L-BFGS driver (artstyletransfer_amd/csrc/nst_lbfgs_host.h) on the host: tests/lbfgs_host.cpp
drives the header alone - vectors of 64 and 257 floats, history capacity 1, 2 and 4, nine pairs (up to 8 evictions) and one
pair with y.s <= 1e-10 dropped at a full history, every dot product formed in double and rounded to float.  After each
pair the incrementally kept SY / YY tables must equal, exactly, tables rebuilt from the surviving pairs, and the direction
formed in double from the fp32 coefficients must be within rel-L2 1e-6 of the fp64 two-loop recursion (the construction
simulated in numpy over both lengths, the three capacities and 20 seeds: worst 5.4e-8; a wrong shift or a transposed SY
entry gives errors of order 1).  Built with AddressSanitizer and UBSan, their runtimes linked into the program; it runs
as a child process, and exit status 0 means every check held."""
import os
import subprocess

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "lbfgs_host.cpp")
CSRC = os.path.join(ROOT, "artstyletransfer_amd", "csrc")


def test_pair_tables_and_direction_coefficients_under_sanitizers(tmp_path):
    exe = str(tmp_path / "lbfgs_host")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", f"-I{CSRC}", SRC, "-o", exe],
                   check=True, capture_output=True, text=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0, r.stdout + r.stderr
    assert "lbfgs host ok: 6 runs" in r.stdout
    print(r.stdout.strip())
