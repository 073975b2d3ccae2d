"""saena_amd/csrc/devmem.h, the owner of the library's device and pinned arrays, on the host: tools/sanitize_devmem.cpp compiles
the header with malloc / free in the place of the HIP calls and checks move, self-move, reset, the refusal of a second alloc and
the live-byte counter under AddressSanitizer and UndefinedBehaviorSanitizer."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_devmem_under_the_sanitizers(tmp_path):
    """a stand-alone program with the sanitizer runtimes linked in statically: it runs in whatever environment the suite runs in"""
    exe = str(tmp_path / "sanitize_devmem")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-DDEVMEM_HOST_TEST", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-static-libasan", "-static-libubsan", os.path.join(ROOT, "tools", "sanitize_devmem.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stdout + b.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("ok"), r.stdout + r.stderr
