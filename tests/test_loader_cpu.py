"""CPU tier of the one loader of the package's shared libraries (svsdct/native.py: load_library, and bind, which gives a binding
module its load() and check()) on three tiny C libraries: one that is right, one that lacks a declared symbol and one that reports
another ABI version; and on a path that does not exist.  Nothing here needs a GPU."""
import ctypes as C
import re
import subprocess

import pytest

from svsdct import native

SIGNATURES = {"stub_abi_version": (C.c_int, []), "stub_last_error": (C.c_char_p, []), "stub_add": (C.c_int, [C.c_int, C.c_int])}
HEAD = 'int stub_abi_version(void) { return %d; }\nconst char *stub_last_error(void) { return "the stub said no"; }\n'
ADD = "int stub_add(int a, int b) { return a + b; }\n"


def _stub(tmp_path, name, text):
    src, so = tmp_path / (name + ".c"), tmp_path / (name + ".so")
    src.write_text(text)
    subprocess.check_call(["gcc", "-shared", "-fPIC", str(src), "-o", str(so)])
    return str(so)


def test_the_loader_and_its_three_refusals(tmp_path, monkeypatch):
    monkeypatch.delenv("SVS_SKIP_ABI_CHECK", raising=False)
    right, lacking, old = (_stub(tmp_path, "right", HEAD % 3 + ADD), _stub(tmp_path, "lacking", HEAD % 3),
                           _stub(tmp_path, "old", HEAD % 2 + ADD))
    lib = native.load_library(right, SIGNATURES, "stub_abi_version", 3)
    assert lib.stub_add(2, 40) == 42 and lib.stub_last_error() == b"the stub said no"
    missing = str(tmp_path / "nowhere.so")
    with pytest.raises(native.SvsNativeError, match=f"libstub.so not found at {re.escape(missing)}; build it with .*There is no CPU fallback"):
        native.load_library(missing, SIGNATURES, "stub_abi_version", 3)
    with pytest.raises(native.SvsNativeError, match=f"{re.escape(lacking)} does not export stub_add; rebuild it"):
        native.load_library(lacking, SIGNATURES, "stub_abi_version", 3)
    with pytest.raises(native.SvsNativeError, match=f"ABI version mismatch: {re.escape(old)} reports 2, the binding expects 3; rebuild libstub.so"):
        native.load_library(old, SIGNATURES, "stub_abi_version", 3)
    monkeypatch.setenv("SVS_SKIP_ABI_CHECK", "1")
    assert native.load_library(old, SIGNATURES, "stub_abi_version", 3).stub_abi_version() == 2
    with pytest.raises(native.SvsNativeError, match="does not export"):       # the escape is for the version alone
        native.load_library(lacking, SIGNATURES, "stub_abi_version", 3)


def test_a_bound_module_loads_once_reads_its_names_at_the_call_and_reports_the_librarys_error(tmp_path):
    right = _stub(tmp_path, "right", HEAD % 3 + ADD)
    module = {"LIB_PATH": str(tmp_path / "nowhere.so"), "SIGNATURES": SIGNATURES, "ABI_VERSION": 3}
    load, check = native.bind(module, "stub")
    with pytest.raises(native.SvsNativeError, match="not found"):
        load()
    module["LIB_PATH"] = right
    assert load() is load() is module["_lib"]
    check(native.SVS_OK, "stub_add")
    with pytest.raises(native.SvsNativeError, match=r"stub_add failed \(-4\): the stub said no") as info:
        check(native.SVS_ERR_CAPACITY, "stub_add")
    assert info.value.code == native.SVS_ERR_CAPACITY
    module["_lib"] = other = object()                  # what tests/testlib.py::using_library does to native._lib
    assert load() is other
