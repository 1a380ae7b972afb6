"""The owner of device memory and the transactional replace helper (artstyletransfer_amd/csrc/nst_devmem.h) on the host:
tests/devmem_host.cpp drives the header alone over malloc / free with an allocator whose k-th request fails, for every k
of a two-level replace - the rollback branches no GPU test can reach without exhausting device memory.  Built with
AddressSanitizer (and its leak check) and UBSan, their runtimes linked into the program; it runs as a child process, and
exit status 0 means every count was exact, nothing leaked, nothing was freed twice and nothing released was touched."""
import os
import subprocess

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "devmem_host.cpp")
CSRC = os.path.join(ROOT, "artstyletransfer_amd", "csrc")


def test_owner_and_replace_helper_under_sanitizers(tmp_path):
    exe = str(tmp_path / "devmem_host")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", f"-I{CSRC}", SRC, "-o", exe],
                   check=True, capture_output=True, text=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0, r.stdout + r.stderr
    assert "devmem ok: 7 replace runs" in r.stdout
