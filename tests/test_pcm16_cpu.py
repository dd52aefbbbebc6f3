"""Sources set as 16-bit PCM (rh_rlm_set_sources_pcm16), the parts that need no GPU: the decision "the rows themselves, or a converted copy"
(rodio_amd/csrc/rh_rlm_pcm16.h) over the cross product of its inputs against the header's conditions written out a second time
(tests/cpp/pcm16_launch_test), the declarations in the header and the binding, the Python mirror's refusal of mixed dtypes, and the entry's
behaviour on a box without a device."""
import ctypes as C
import importlib.util
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "pcm16_launch_test")


def pcm16_launch_exe():
    if not os.path.exists(EXE):  # build() makes it; a tree built before this driver existed gets it here
        spec = importlib.util.spec_from_file_location("_rh_build", os.path.join(ROOT, "rodio_amd", "build.py"))
        b = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(b)
        b.build_driver("pcm16_launch_test", False, lambda cmd: subprocess.check_call(cmd))
    return EXE


def test_native_or_converted_over_the_cross_product():
    r = subprocess.run([pcm16_launch_exe()], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr + r.stdout
    words = r.stdout.split()
    n = {k: int(v) for k, v in zip(words[::2], words[1::2])}
    assert n["failures"] == 0
    # not vacuous: both answers for both native routes (and for no other), every reason for converting reached
    assert n["decisions"] > 100_000
    assert n["routes_native"] == 2 and n["routes_both"] == 2
    assert n["reasons_reached"] == n["reasons"] == 6


def test_header_and_binding_declare_both_entries(rh):
    from rodio_amd import _lib

    text = open(os.path.join(ROOT, "include", "rodio_hip.h")).read()
    assert re.search(r"rh_status rh_rlm_set_sources_pcm16\(rh_rlm \*p, const int16_t \*const \*srcs_host, const uint64_t \*in_frames_host, uint32_t n_sources\);", text)
    assert re.search(r"rh_status rh_rlm_source_format\(rh_rlm \*p, int32_t \*format, int32_t \*native\);", text)
    assert _lib.SIGNATURES["rh_rlm_set_sources_pcm16"] == _lib.SIGNATURES["rh_rlm_set_sources"]
    assert len(_lib.SIGNATURES["rh_rlm_source_format"][1]) == 3
    assert _lib.lib.rh_rlm_set_sources_pcm16 and _lib.lib.rh_rlm_source_format
    # the comment says which runs are native, what they need of the rows, and that everything else converts once
    doc = text[text.index("srcs_host[s] = device pointer of source s as interleaved signed 16-bit PCM"):text.index("rh_status rh_rlm_set_sources_pcm16")]
    for must in ("k_rlm_chunk_pcm16", "k_mix_rows_pcm16", "16-byte boundary", "8-byte boundary", "frames * channels % 8 == 0", "ONCE per rh_rlm_set_sources_pcm16", "RH_ERR_NOMEM"):
        assert must in doc, must


class _Spy:
    """Stands in for the library: any call is an error."""

    def __getattr__(self, name):
        raise AssertionError(f"library call {name} before the dtypes were checked")


def test_set_sources_refuses_mixed_and_foreign_dtypes_before_any_library_call(rh, monkeypatch):
    import torch

    from rodio_amd import source

    p = source.ResampleLowpassMix.__new__(source.ResampleLowpassMix)  # (no handle: nothing here may reach the library)
    p._h, p.channels, p._keep, p.out_frames = C.c_void_p(), 2, None, 0
    monkeypatch.setattr(source, "lib", _Spy())
    f32, i16 = torch.zeros(8, dtype=torch.float32), torch.zeros(8, dtype=torch.int16)
    with pytest.raises(ValueError):
        p.set_sources([f32, i16])
    with pytest.raises(ValueError):
        p.set_sources([i16, i16, f32])
    for other in (torch.float64, torch.int32, torch.uint8, torch.float16):
        with pytest.raises(ValueError):
            p.set_sources([torch.zeros(8, dtype=other)])
    with pytest.raises(AssertionError, match="rh_rlm_set_sources_pcm16"):  # int16 rows go to the new entry ...
        p.set_sources([i16, i16])
    with pytest.raises(AssertionError, match="rh_rlm_set_sources before"):  # ... f32 rows to the one they always took
        p.set_sources([f32, f32])


def test_no_device_no_fallback(rh):
    import torch

    if torch.cuda.is_available():
        return  # covered by the gpu tests
    from rodio_amd import _lib

    lib = _lib.lib
    assert lib.rh_init(0) == 2  # RH_ERR_HIP: no device
    rows = (C.c_void_p * 1)(None)
    frames = (C.c_uint64 * 1)(0)
    fmt, nat = C.c_int32(7), C.c_int32(7)
    # RH_ERR_NOT_INITIALIZED (6), exactly as rh_rlm_set_sources answers: no handle can exist, and nothing is computed on the host instead
    assert lib.rh_rlm_set_sources(None, rows, frames, 1) == 6
    assert lib.rh_rlm_set_sources_pcm16(None, rows, frames, 1) == 6
    assert lib.rh_rlm_source_format(None, C.byref(fmt), C.byref(nat)) == 1  # RH_ERR_INVALID: no handle
    assert (fmt.value, nat.value) == (7, 7)
