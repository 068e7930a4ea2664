"""The exact solver's opening book without a GPU.

* tests/native/book_check.cpp, built here with -fsanitize=address,undefined:
  the host build of csrc/az_book.h's per-position functions (mirror, canonical
  key, decode, the child test, the retrograde value), a book built from them
  against a plain negamax on 4x4, the canonical level counts, the file.
* exact_solvers.get_solver(): with ConfigSolver.book_path == "" no book
  function is called; with a path, the file is loaded, and a missing file, a
  refused file and an unfinished book each raise an error that says which.
* hipcc's resource remarks for az_book.hip's own kernels: no scratch, no
  spilled VGPR.
"""
import os
import re
import subprocess

import pytest

from custom_alphazero import engine as az
from custom_alphazero.config import ConfigConnectN, ConfigSolver
from custom_alphazero.exact_solvers import c4_exact_solver as exact

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(REPO, "tests", "native")
CSRC = os.path.join(REPO, "custom-alphazero_amd", "csrc")
EXE = os.path.join(NATIVE, "_build", "book_check")
HIPCC = "/opt/rocm/bin/hipcc"
KERNELS = ["expand_kernel", "retro_kernel", "lookup_kernel", "level_kernel", "pick_kernel", "store_kernel"]


def test_host_build_of_the_book_functions(tmp_path):
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    subprocess.run([os.environ.get("CXX", "g++"), "-O2", "-g", "-std=c++17", "-Wall",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(NATIVE, "book_check.cpp"), "-o", EXE], check=True, timeout=600)
    out = subprocess.run([EXE, str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    assert out.stdout.splitlines()[-1] == "ok"


# ------------------------------------------------------------------ get_solver on a stub
class StubSolver:
    """engine.Solver's surface as get_solver uses it; records every call.
    load_error (raised by book_load) and state (book_info's) are set on the class."""
    made, load_error, state = [], None, az.BOOK_FINISHED

    def __init__(self, height, width, n, tt_log2=24, device=0):
        self.geometry, self.calls, self.closed = (height, width, n), [], False
        StubSolver.made.append(self)

    def configure(self, **kw):
        self.calls.append("configure")

    def close(self):
        self.closed = True

    def book_load(self, path):
        self.calls.append(("book_load", path))
        if StubSolver.load_error:
            raise StubSolver.load_error

    def book_info(self):
        self.calls.append("book_info")
        return 6, StubSolver.state, [1] * 7

    def __getattr__(self, name):
        if name.startswith("book_"):
            raise AssertionError(f"{name} called")
        raise AttributeError(name)


@pytest.fixture
def stub(monkeypatch):
    monkeypatch.setattr(ConfigConnectN, "board_width", 5)
    monkeypatch.setattr(ConfigConnectN, "board_height", 4)
    monkeypatch.setattr(ConfigConnectN, "n", 4)
    monkeypatch.setattr(ConfigConnectN, "gravity", True)
    monkeypatch.setattr(ConfigSolver, "node_budget", 1000)
    monkeypatch.setattr(exact.az, "Solver", StubSolver)
    monkeypatch.setattr(exact, "_solvers", {})
    StubSolver.made, StubSolver.load_error, StubSolver.state = [], None, az.BOOK_FINISHED
    return StubSolver


def test_no_book_path_no_book_call(stub):
    assert ConfigSolver.book_path == ""
    s = exact.get_solver()
    assert exact.get_solver() is s and len(stub.made) == 1
    assert s.geometry == (4, 5, 4) and s.calls == ["configure"]


def test_book_path_is_loaded_once(stub, monkeypatch, tmp_path):
    path = tmp_path / "a.book"
    path.write_bytes(b"x")
    monkeypatch.setattr(ConfigSolver, "book_path", str(path))
    s = exact.get_solver()
    assert exact.get_solver() is s
    assert s.calls == ["configure", ("book_load", str(path)), "book_info"]
    monkeypatch.setattr(ConfigSolver, "book_path", "")  # another setting, another solver: the book is not kept
    assert exact.get_solver() is not s and stub.made[-1].calls == ["configure"]


def test_book_path_errors_say_which(stub, monkeypatch, tmp_path):
    missing = str(tmp_path / "none.book")
    monkeypatch.setattr(ConfigSolver, "book_path", missing)
    with pytest.raises(FileNotFoundError, match="none.book"):
        exact.get_solver()
    assert not stub.made  # refused before a solver is made
    path = tmp_path / "a.book"
    path.write_bytes(b"x")
    monkeypatch.setattr(ConfigSolver, "book_path", str(path))
    stub.load_error = az.AzError("az_solver_book_load: another geometry: the file is 4x4 n=4, the solver 5x4 n=4")
    with pytest.raises(az.AzError, match="another geometry"):
        exact.get_solver()
    assert stub.made[-1].closed and not exact._solvers
    stub.load_error, stub.state = None, az.BOOK_BUILDING
    with pytest.raises(RuntimeError, match="not finished"):
        exact.get_solver()
    assert stub.made[-1].closed and not exact._solvers


def test_binding_lists_the_book_functions():
    names = ["az_solver_book_begin", "az_solver_book_solve", "az_solver_book_finish", "az_solver_book_save",
             "az_solver_book_load", "az_solver_book_info", "az_solver_book_level"]
    assert all(n in az.EXPORTED for n in names)
    L = az.load_library()
    assert all(hasattr(L, n) for n in names) and L.az_abi_version() == 10


# ------------------------------------------------------------------ kernel resources
@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_book_kernels_use_no_scratch(tmp_path):
    out = subprocess.run(
        [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Rpass-analysis=kernel-resource-usage",
         "-c", os.path.join(CSRC, "az_book.hip"), "-o", str(tmp_path / "b.o")],
        capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    usage, name = {}, None
    for line in out.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            usage[name] = {}
        m = re.search(r"(VGPRs Spill|ScratchSize \[bytes/lane\]): (\d+)", line)
        if m and name:
            usage[name][m.group(1)] = int(m.group(2))
    for kernel in KERNELS:
        found = {k: v for k, v in usage.items() if "4book" in k and kernel in k}
        assert len(found) == 1, (kernel, sorted(usage))
        for k, v in found.items():
            assert v == {"VGPRs Spill": 0, "ScratchSize [bytes/lane]": 0}, (k, v)
