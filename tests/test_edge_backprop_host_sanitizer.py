"""Host side of the entry points of csrc/edge_backprop.hip and gode_edge_ode_feval_save_f32 - argument validation and
marshalling - under the address and undefined-behaviour sanitizers: a stand-alone program with its own main
(tests/native/edge_backprop_host_check.cpp), built from the two sources with the sanitizers on the host code only and run
on the CPU.  Nothing loaded into python runs under a sanitizer, and no kernel is launched."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = "-fsanitize=address,undefined"


def test_host_side_of_the_entry_points_under_asan_and_ubsan(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc), "hipcc is needed to build the library, hence this check"
    csrc = os.path.join(ROOT, "graph_odenet_amd", "csrc")
    sources = [os.path.join(ROOT, "tests", "native", "edge_backprop_host_check.cpp"),
               os.path.join(csrc, "edge_backprop.hip"), os.path.join(csrc, "edge_ode.hip")]
    objs = []
    for src in sources:
        obj = str(tmp_path / (os.path.basename(src) + ".o"))
        subprocess.run([hipcc, "-O1", "-g", "-std=c++17", "--offload-arch=gfx950", "-Xarch_host", SAN, "-Xarch_host",
                        "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-I" + os.path.join(ROOT, "include"),
                        "-x", "hip", "-c", src, "-o", obj], check=True)
        objs.append(obj)
    prog = str(tmp_path / "edge_backprop_host_check")
    subprocess.run([hipcc, "--offload-arch=gfx950", SAN] + objs + ["-o", prog], check=True)
    assert b"__asan_init" in open(prog, "rb").read(), "the program was not linked against the sanitizer runtime"
    res = subprocess.run([prog], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "host check ok" in res.stdout and "runtime error" not in res.stderr and "AddressSanitizer" not in res.stderr
