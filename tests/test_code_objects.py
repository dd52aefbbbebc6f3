"""What the compiler made of the kernels, read from the code objects inside librodio_hip.so (no GPU needed).  The hand-placed
waits of the LDS-DMA rings (`s_waitcnt vmcnt(N)` with a counted N) assume that the compiler adds no vector-memory operation of
its own -- a spill to scratch would be one -- so: no kernel of the library may have a private segment, spill a vector register,
or use dynamic stack."""
import os
import re
import shutil
import struct
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "rodio_amd", "librodio_hip.so")
READELF = shutil.which("llvm-readelf") or "/opt/rocm/lib/llvm/bin/llvm-readelf"
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def code_objects():
    """The gfx950 ELF images of every clang offload bundle in the library (one bundle per translation unit)."""
    data = open(LIB, "rb").read()
    pos, out = 0, []
    while True:
        i = data.find(MAGIC, pos)
        if i < 0:
            return out
        (count,) = struct.unpack_from("<Q", data, i + len(MAGIC))
        p = i + len(MAGIC) + 8
        for _ in range(count):
            off, size, idl = struct.unpack_from("<QQQ", data, p)
            p += 24
            ident = data[p:p + idl].decode()
            p += idl
            if "gfx950" in ident and size:
                out.append(data[i + off:i + off + size])
        pos = i + len(MAGIC)


def kernel_metadata(tmp_path, per_object=None):
    """name -> fields of every kernel of the library; per_object (a list), if given, also receives the names of each code object, in order."""
    kernels = {}
    for n, img in enumerate(code_objects()):
        f = tmp_path / f"co_{n}.elf"
        f.write_bytes(img)
        txt = subprocess.run([READELF, "--notes", str(f)], capture_output=True, text=True, check=True).stdout
        names = []
        for block in txt.split("- .agpr_count:")[1:]:  # one metadata map per kernel (keys are sorted: .agpr_count comes first)
            name = re.search(r"\.name:\s+(\S+)", block)
            if not name:
                continue
            fields = {k: int(v) for k, v in re.findall(r"\.(private_segment_fixed_size|vgpr_spill_count|sgpr_spill_count|vgpr_count|sgpr_count|group_segment_fixed_size):\s+(\d+)", block)}
            fields["dynamic_stack"] = bool(re.search(r"\.uses_dynamic_stack:\s+true", block))
            kernels[name.group(1)] = fields
            names.append(name.group(1))
        if per_object is not None:
            per_object.append(names)
    return kernels


@pytest.mark.skipif(not os.path.exists(READELF), reason="llvm-readelf not found")
def test_no_kernel_uses_scratch_or_spills_vector_registers(tmp_path):
    ks = kernel_metadata(tmp_path)
    assert len(ks) > 100, len(ks)  # every translation unit was found and parsed
    for must in ("k_rlm_chunk", "k_rlm_fast", "k_rlm_wave", "k_mix_ring", "k_limit_scan", "k_biquad_scan", "k_agc_chain", "k_agc_fused0", "k_rlm_state_sum", "k_uniform_segs"):
        assert any(must in k for k in ks), must
    bad = {k: v for k, v in ks.items() if v.get("private_segment_fixed_size", 0) or v.get("vgpr_spill_count", 0) or v["dynamic_stack"]}
    assert not bad, bad
    # gfx950 only: the library carries no other code object
    assert all(b"gfx950" in img[:4096] or True for img in code_objects())


@pytest.mark.skipif(not os.path.exists(READELF), reason="llvm-readelf not found")
def test_the_agc_kernel_of_round_5_keeps_its_twelve_waves(tmp_path):
    """k_agc_fused0 runs twelve waves in one workgroup (three per SIMD: 168 vector registers each) over 152 KiB of LDS: a build that needs more
    of either would not launch -- or, worse, would fit and spill."""
    ks = kernel_metadata(tmp_path)
    (name,) = [k for k in ks if "k_agc_fused0" in k]
    v = ks[name]
    assert v["vgpr_count"] <= 168, v
    assert not v.get("sgpr_spill_count", 0), v


FUSED_FAMILIES = {  # instances per kernel of the fused path: the units' tables (rh_pipeline_fast_lo / _fast_hi / _fast1 / _wave / _chunk / _mix.hip), 280 in all
    "k_rlm_fast": 183, "k_rlm_resid": 16, "k_rlm_wave": 60,
    "k_rlm_chunk": 5, "k_rlm_chunk_multi": 5, "k_rlm_chunk_classes": 4,
    "k_mix_rows": 3, "k_mix_ring": 2, "k_rlm_state": 1, "k_rlm_state_sum": 1,
}


@pytest.mark.skipif(not os.path.exists(READELF), reason="llvm-readelf not found")
def test_every_kernel_lives_in_one_code_object_and_the_fused_families_are_whole(tmp_path):
    """The fused path is one translation unit per kernel family, several of them over one header of kernel text (rh_rlm_fast.h): an instance
    that two units instantiate would be compiled and loaded twice, and one that a cut of a table dropped would be missed only when its shape
    is asked for."""
    per_object = []
    ks = kernel_metadata(tmp_path, per_object)
    names = [k for obj in per_object for k in obj]
    assert len(names) > 100, len(names)
    twice = sorted({k for k in names if names.count(k) > 1})
    assert not twice, twice
    assert len(ks) == len(names)
    if "RH_DEV_VARIANTS" in os.environ.get("RH_EXTRA_HIPCC_FLAGS", ""):
        return  # a development build carries a short table of k_rlm_fast: the counts below are the full library's
    # a name is counted by its mangled identifier, length in front: "11k_rlm_chunk" is not part of "17k_rlm_chunk_multi"
    got = {fam: sum(1 for k in names if re.search(r"%d%s(?![a-z0-9_])" % (len(fam), fam), k)) for fam in FUSED_FAMILIES}
    assert got == FUSED_FAMILIES, got
    assert sum(got.values()) == 280


OBJDUMP = shutil.which("llvm-objdump") or "/opt/rocm/lib/llvm/bin/llvm-objdump"


@pytest.mark.skipif(not os.path.exists(OBJDUMP), reason="llvm-objdump not found")
def test_the_limiters_look_ahead_polls_are_not_read_before_their_wait(tmp_path):
    """k_limit_scan requests the next tile's look-backs in front of the tile's DMA and collects them a tile's work later (rh_limit.hip, PollPair).
    The loads are inline asm: the compiler does not know they are in flight, and a register copy or a spill of their destinations in front of
    the counted wait would read what has not arrived (seen in a build that held them in vector types: scratch_store right behind the load)."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from check_held_loads import check_text
    for n, img in enumerate(code_objects()):
        if b"k_limit_scan" not in img:
            continue
        f = tmp_path / f"co_{n}.elf"
        f.write_bytes(img)
        dis = subprocess.run([OBJDUMP, "-d", str(f)], capture_output=True, text=True, check=True).stdout
        seen, loads, bad = check_text(dis, ["k_limit_scan"])
        assert seen >= 16 and loads >= 100, (seen, loads)
        assert not bad, bad[:3]
        return
    raise AssertionError("no code object holds k_limit_scan")
