"""CPU-side check of what the add-on bindings share (zen_amd/_addon.py: Library, Owner / Profiled / Handle) against a library
of counters compiled from tests/cpp/fake_addon.c with the host compiler: no HIP library, no device."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class Stats(C.Structure):
    _fields_ = [("created", C.c_ulonglong), ("destroyed", C.c_ulonglong), ("streams", C.c_ulonglong), ("profiling", C.c_int)]


_i, _vp, _pd, _pull = C.c_int, C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_ulonglong)
SYMBOLS = [
    ("zen_hip_fake_last_error", C.c_char_p, []),
    ("zen_hip_fake_fail", _i, [_i]),
    ("zen_hip_fake_create", _i, [_i, C.POINTER(_vp)]),
    ("zen_hip_fake_destroy", _i, [_vp]),
    ("zen_hip_fake_set_stream", _i, [_vp, _vp]),
    ("zen_hip_fake_stats", _i, [_vp, C.POINTER(Stats)]),
    ("zen_hip_fake_profile", _i, [_vp, _i]),
    ("zen_hip_fake_profile_get", _i, [_vp, _pd, _pull, _pull]),
]
KERNELS = ("zeta", "alpha", "mid")      # not sorted: profile_get keeps this order


@pytest.fixture
def fake(tmp_path, monkeypatch):
    """(the Library of libzen_hip_fake.so, a Handle class on it); the engine library's loader patched out"""
    from zen_amd import _addon, lib
    so = str(tmp_path / "libzen_hip_fake.so")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-shared", "-fPIC", os.path.join(ROOT, "tests", "cpp", "fake_addon.c"),
                           "-o", so])
    monkeypatch.setenv("ZEN_HIP_FAKE_SO", so)
    monkeypatch.setattr(lib, "load", lambda: None)
    library = _addon.Library("fake", SYMBOLS, zg_codes=(3,), kernels=KERNELS, stats=Stats)

    class Fake(_addon.Handle):
        _lib = library

        def __init__(self, rc=0):
            self._create(rc)
    yield library, Fake
    _addon._libs.pop("fake", None)


def test_handle_base_against_a_library_of_counters(fake, monkeypatch):
    from zen_amd import _addon, lib
    library, Fake = fake

    def counts():
        st = Stats()
        assert library.fn("stats")(None, C.byref(st)) == 0
        return st.created, st.destroyed
    assert library.fn("create") is library.load().zen_hip_fake_create and counts() == (0, 0)

    # destroy exactly once per handle: when the object goes ...
    a = Fake()
    assert a._h and a._L is library.load() and counts() == (1, 0)
    del a
    assert counts() == (1, 1)
    # ... or at the explicit close, and not again when the object goes after it
    b = Fake()
    b._close()
    assert b._h is None and counts() == (2, 2)
    b._close()
    del b
    assert counts() == (2, 2)
    # a create that failed leaves nothing to destroy
    with pytest.raises(lib.ZenHipError, match="zen_hip error 2: fake_create: refused") as e:
        Fake(rc=2)
    assert type(e.value) is lib.ZenHipError and e.value.code == 2
    del e
    assert counts() == (2, 2)

    # check: ZgException for the listed codes, ZenHipError for the others, the library's own message in both; 0 passes
    assert library.check(0) is None
    with pytest.raises(lib.ZenHipError, match="zen_hip error 5: fake_fail: as asked") as e:
        library.check(library.fn("fail")(5))
    assert type(e.value) is lib.ZenHipError
    with pytest.raises(lib.ZgException, match="zen_hip error 3: fake_fail: as asked"):
        library.check(library.fn("fail")(3))
    with pytest.raises(lib.ZgException, match="zen_hip error 3: fake_create: refused"):
        Fake(rc=3)

    # what every handle answers
    h = Fake()
    h.set_stream(None)
    h.set_stream(1234)
    h.profile()
    assert h.stats() == {"created": 3, "destroyed": 2, "streams": 2, "profiling": 1}
    h.profile(False)
    assert h.stats()["profiling"] == 0
    got = h.profile_get()
    assert list(got) == list(KERNELS)
    assert got == {"zeta": {"ms": 0.5, "bytes": 100, "launches": 1}, "alpha": {"ms": 1.5, "bytes": 200, "launches": 2},
                   "mid": {"ms": 2.5, "bytes": 300, "launches": 3}}
    h._close()
    with pytest.raises(lib.ZenHipError, match="fake_set_stream: null handle"):
        h.set_stream(None)
    assert counts() == (3, 3)

    # an override that names no file: ImportError, nothing built in its place
    _addon._libs.pop("fake")
    monkeypatch.setenv("ZEN_HIP_FAKE_SO", os.path.join(os.path.dirname(os.environ["ZEN_HIP_FAKE_SO"]), "absent.so"))
    with pytest.raises(ImportError, match="absent.so does not exist"):
        library.load()
