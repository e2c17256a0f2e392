"""csrc/sr_view.h -- the acceptance rules of the convolution entry points -- is plain C: tests/host/view_checks.c includes it,
checks the predicates at their boundaries and is compiled here the way oracle/Makefile compiles the oracle (gcc, no HIP)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_view_predicates_at_their_boundaries(tmp_path):
    exe = str(tmp_path / "view_checks")
    cc = os.environ.get("CC", "gcc")
    subprocess.run([cc, "-std=c99", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "simplerecon_amd", "csrc"),
                    "-o", exe, os.path.join(ROOT, "tests", "host", "view_checks.c")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "view checks ok", r.stdout + r.stderr
