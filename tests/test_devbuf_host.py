"""Who owns the engine's device memory, checked on the host: tools/devbuf_check.cpp runs the stage structs of
ces_amd/csrc/cesx_stages.h over a malloc-backed dev_alloc / dev_free whose calls fail in turn.  Built with the host
compiler alone -- no ROCm include path, so the build is also the check that devbuf.h and cesx_stages.h are free of hip/."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENARIOS = 33          # 5 per stage struct (6 of them), the Lorenz '96 re-install, DevBuf itself, Engine::core


def test_stage_structs_free_what_they_own(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "devbuf_check")
    build = subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tools", "devbuf_check.cpp")],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    lines = run.stdout.splitlines()
    assert sum(ln.startswith("ok ") for ln in lines) == SCENARIOS, run.stdout
    assert not any(ln.startswith("FAILED") for ln in lines)
    assert lines[-1] == "%d scenarios, all ok" % SCENARIOS
    for who in ("MhState", "GpState", "GpDenseState", "GpFitState", "DarcyState", "L96State", "DevBuf", "core"):
        assert any(ln.startswith("ok %s:" % who) for ln in lines), who
