"""The arena layout arithmetic and the row lists the host-pointer entry points stage by (fp_layout.h, fp_rows.h),
without a GPU: tests/layout_host_main.cc is built as a stand-alone program under AddressSanitizer and
UndefinedBehaviorSanitizer and run.  It stages every row list into a heap block of exactly the total the layout
reports, so a total that forgets an array is a heap overflow, and compares the totals of
fp_place_batch_policy_quota (every option given) and fp_drain_sweep with the byte formulas they replaced."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# the sanitizer runtimes are linked statically, so that the program needs nothing from its environment
COMPILERS = [("g++", ["-static-libasan", "-static-libubsan"]), ("c++", ["-static-libasan", "-static-libubsan"]),
             ("clang++", []), ("/opt/rocm/llvm/bin/clang++", []), ("/opt/rocm/lib/llvm/bin/clang++", [])]


def _build(src, exe):
    log = []
    for cxx, extra in COMPILERS:
        path = shutil.which(cxx)
        if not path:
            continue
        r = subprocess.run([path, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", *extra, src, "-o", exe],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, cwd=ROOT)
        if r.returncode == 0:
            return
        log.append(f"{path}: {r.stdout}")
    raise AssertionError("no host C++ compiler built the program:\n" + "\n".join(log))


def test_layout_under_sanitizers(tmp_path):
    exe = str(tmp_path / "layout_host")
    _build(os.path.join(ROOT, "tests", "layout_host_main.cc"), exe)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout
    assert r.stdout.rstrip().endswith("layout ok")
    assert "policy S=3 C=3000 N=700" in r.stdout and "drain C=3000 N=700" in r.stdout
    assert "order grow_policy: 0 2 4 " in r.stdout and "order replan: 0 3 6 " in r.stdout
