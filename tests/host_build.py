"""What the test_*_host.py modules share: the host C++ compiler, and building project sources for the CPU - as a shared object that
ctypes loads, or as a stand-alone program with its own main, plain or under AddressSanitizer and UndefinedBehaviorSanitizer.  The
sanitized runs are runs of stand-alone programs: nothing sanitized is ever loaded into the Python process."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "tests", "host")
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
THREAD_SANITIZE = ["-fsanitize=thread"]


def host_cxx(gcc=False):
    """the host C++ compiler, or skip: ROCm's clang++ or the one on the path (sources that use ext_vector_type need clang); gcc: g++ will do too"""
    names = ["/opt/rocm/lib/llvm/bin/clang++", shutil.which("clang++") or ""] + ([shutil.which("g++") or ""] if gcc else [])
    c = next((c for c in names if c and os.path.exists(c)), None)
    if not c:
        pytest.skip("no C++ compiler" if gcc else "no clang++")
    return c


def build_shared(cxx, sources, so):
    """the sources as a shared object for ctypes; returns its path"""
    so = str(so)
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-fPIC", "-shared"] + _list(sources) + ["-o", so])
    return so


def build_program(cxx, sources, exe, defines=(), extra=()):
    """the sources as a stand-alone program; returns the compiler's CompletedProcess"""
    return subprocess.run([cxx, "-O1", "-g", "-std=c++17"] + ["-D" + d for d in defines] + list(extra) + _list(sources) + ["-o", str(exe)],
                          capture_output=True, text=True)


def sanitizers_work(cxx, tmp_path, flags=SANITIZE):
    """whether an empty program builds and runs under the sanitizers here, i.e. their runtimes are installed"""
    probe_src, probe = str(tmp_path / "probe.cpp"), str(tmp_path / "probe")
    open(probe_src, "w").write("int main() { return 0; }\n")
    p = subprocess.run([cxx] + list(flags) + [probe_src, "-o", probe], capture_output=True, text=True)
    return not p.returncode and not subprocess.run([probe], capture_output=True).returncode


def run_program(cxx, sources, exe, args=(), defines=(), sanitized=False, extra=(), timeout=None):
    """Builds the stand-alone program `exe` (a path under the test's tmp_path) and runs it; returns the run's CompletedProcess.  The
    build failing is a failure.  sanitized: under the sanitizers - True for SANITIZE, or a set of flags of the caller's such as
    THREAD_SANITIZE - skipped only where an empty program does not build and run under them; a failure of the project's source is a
    failure.  extra: further compiler flags.  timeout: seconds the run may take; running out of them is a failure."""
    flags = SANITIZE if sanitized is True else list(sanitized or ())
    if flags and not sanitizers_work(cxx, exe.parent, flags):
        pytest.skip("the sanitizer runtimes are not installed")
    r = build_program(cxx, sources, exe, defines, list(flags) + list(extra))
    assert r.returncode == 0, r.stderr[-2000:]
    try:
        return subprocess.run([str(exe)] + [str(a) for a in args], capture_output=True, text=True, timeout=timeout)
    except subprocess.TimeoutExpired:
        pytest.fail("%s did not finish within %s s" % (os.path.basename(str(exe)), timeout))


def _list(sources):
    return [sources] if isinstance(sources, str) else list(sources)


def library():
    """the av1mi module over the built library, for tests of its host-only entry points; builds the library first where it is missing"""
    if not os.path.exists(os.path.join(ROOT, "av1-base_amd", "libav1mi.so")):
        import importlib.util
        spec = importlib.util.spec_from_file_location("av1mi_build", os.path.join(ROOT, "av1-base_amd", "build.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        mod.build()
    import av1mi as m
    return m
