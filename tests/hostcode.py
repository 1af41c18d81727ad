"""The kernels' code built for the host with the system compiler: the compiler lookup, a shared object loaded through ctypes, and a
stand-alone program (the source's own main) under the address and undefined-behaviour sanitizers.  Every caller passes its own flags and
time limits; nothing here puts a sanitizer's runtime into the python process."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

SANITIZE = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def _compiler():
    for name in (os.environ.get("CXX"), "c++", "g++", "clang++"):
        path = name and shutil.which(name)
        if path:
            return path
    return None


def _compiler_or_skip():
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler")
    return cxx


def _vp(a):
    """A numpy array (or None) as the void pointer a host-built function takes."""
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def load_shared(tmp_path, name, flags, timeout):
    """`flags` (the sources among them) compiled into tmp_path/name.so -> the loaded library."""
    so = str(tmp_path / (name + ".so"))
    b = subprocess.run([_compiler_or_skip()] + flags + ["-o", so], capture_output=True, text=True, timeout=timeout)
    assert b.returncode == 0, b.stderr[-3000:]
    return C.CDLL(so)


def run_sanitized(tmp_path, name, flags, probe_timeout, build_timeout, run_timeout):
    """`flags` (a define that selects the source's main among them) compiled under SANITIZE into the program tmp_path/name and run -> the
    finished run, which has returned 0; the caller looks at what it wrote."""
    cxx = _compiler_or_skip()
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run([cxx] + SANITIZE + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True, timeout=probe_timeout).returncode != 0:
        pytest.skip("the compiler lacks the sanitizers' runtimes")
    exe = str(tmp_path / name)
    b = subprocess.run([cxx] + SANITIZE + flags + ["-o", exe], capture_output=True, text=True, timeout=build_timeout)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=run_timeout)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    return r
