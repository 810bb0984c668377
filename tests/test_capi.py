"""The C-ABI library loads and exports every entry point include/msv.h declares; host-only calls
behave; device calls fail with a status (never a crash) when no GPU is visible.  CPU only."""
import ctypes as C
import os
import re
import subprocess

import pytest

from hmm_fasta_viterbi_amd import _native
from oracle_lib import ROOT


def declared_functions():
    text = open(os.path.join(ROOT, "include", "msv.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(msv_[a-z0-9_]+)\s*\(", text)))


def test_header_declares_the_bound_symbols():
    assert declared_functions() == sorted(_native.EXPORTED)


def test_library_exports_every_declared_symbol():
    out = subprocess.run(["nm", "-D", "--defined-only", _native.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    exported = set(re.findall(r"\bT (msv_[a-z0-9_]+)$", out, flags=re.M))
    missing = [f for f in declared_functions() if f not in exported]
    assert not missing, missing
    L = _native.lib()
    for f in declared_functions():
        assert getattr(L, f) is not None


def test_status_strings_and_version():
    L = _native.lib()
    for code, name in _native.STATUS.items():
        assert L.msv_status_string(code).decode() == name
    assert b"gfx950" in L.msv_version()


def test_kernel_family_is_gfx950_code_object(tmp_path):
    # llvm-objdump --offloading extracts the bundled code objects next to its input: work on a copy
    import shutil
    lib = shutil.copy(_native.LIB_PATH, tmp_path / "libmsv_hip.so")
    out = subprocess.run(["/opt/rocm/lib/llvm/bin/llvm-objdump", "--offloading", "-h", str(lib)],
                         capture_output=True, text=True)
    blob = out.stdout + out.stderr
    assert "gfx950" in blob or "hipv4-amdgcn-amd-amdhsa--gfx950" in open(lib, "rb").read().decode("latin-1")


def test_invalid_arguments_return_status():
    L = _native.lib()
    p = C.c_void_p()
    assert L.msv_profile_create(0, None, 101, 0.0, 0.0, 0.0, C.byref(p)) == 1
    assert L.msv_score_batch(None, None, None, 0, None, None) == 1
    assert L.msv_hmm_read(None, C.byref(p)) == 1


@pytest.mark.skipif(os.environ.get("HIP_VISIBLE_DEVICES") is None and os.path.exists("/dev/kfd"),
                    reason="a GPU may be present")
def test_no_device_is_a_status_not_a_crash():
    L = _native.lib()
    n = C.c_int(-1)
    L.msv_device_count(C.byref(n))
    if n.value == 0:
        import numpy as np
        es = np.zeros(20 * 101, np.float32)
        p = C.c_void_p()
        assert L.msv_profile_create(0, es.ctypes.data, 101, -8.5, -0.69, -0.69, C.byref(p)) == 7


def test_host_only_entry_points_validate_arguments():
    """Host-side C-ABI calls added after the first round of the API (grid, multi-device, P-values,
    shard bounds, GPU FASTA) reject bad arguments with a status and never touch a device."""
    import numpy as np
    L = _native.lib()
    out = np.zeros(4, np.uint64)
    offs = np.array([0, 3, 3, 10], np.uint64)
    assert L.msv_shard_bounds(None, 3, 2, out.ctypes.data) == 1          # offsets NULL with n > 0
    assert L.msv_shard_bounds(offs.ctypes.data, 3, 0, out.ctypes.data) == 1  # zero shards
    assert L.msv_shard_bounds(offs.ctypes.data, 3, 3, out.ctypes.data) == 0
    assert list(out) == [0, 0, 2, 3]  # cut k: first sequence whose end reaches k/3 of the residues
    assert L.msv_shard_bounds(offs.ctypes.data, 0, 3, out.ctypes.data) == 0 and list(out) == [0, 0, 0, 0]
    pv = np.zeros(3, np.float64)
    bad_offs = np.array([0, 5, 2, 9], np.uint64)                          # decreasing offsets
    sc = np.zeros(3, np.float32)
    assert L.msv_pvalues(sc.ctypes.data, bad_offs.ctypes.data, 3, -9.0, 0.7, pv.ctypes.data) == 1
    assert L.msv_pvalues(None, None, 0, -9.0, 0.7, None) == 0             # empty batch
    assert L.msv_score_grid(None, 0, None, None, 0, None, None) == 1
    assert L.msv_score_batch_multi(None, 0, None, None, 0, None) == 1
    f = C.c_void_p()
    assert L.msv_fasta_parse_device(0, None, 10, None, C.byref(f)) == 1  # text NULL with n > 0
    assert L.msv_fasta_read_device(0, None, None, C.byref(f)) == 1
    assert L.msv_fasta_device_count(None) == 0 and L.msv_fasta_device_codes(None) is None
    assert L.msv_score_fasta_device(None, None, None) == 1
    assert L.msv_fasta_device_device(None) == -1  # no set: no device


def test_viterbi_entry_points_validate_arguments():
    """a positive transition score (the kernel leaves D(LENG) out of E, exact only for
    transitions <= 0) and a NULL stream for msv_filter_select_device (the legacy null stream, unordered
    with the profiles' non-blocking streams) are rejected before any device is touched."""
    import numpy as np
    L = _native.lib()
    M = 101
    msc = np.zeros((20, M), np.float32)
    tsc = np.full((M, 7), np.float32(np.log(np.float32(0.5))), np.float32)
    tsc[5, 3] = 0.25  # node 5, i->m
    p = C.c_void_p()
    assert L.msv_vit_profile_create(0, msc.ctypes.data, None, tsc.ctypes.data, M, -8.0, -0.69, -0.69,
                                    C.byref(p)) == 1
    tsc[5, 3] = np.nan
    assert L.msv_vit_profile_create(0, msc.ctypes.data, None, tsc.ctypes.data, M, -8.0, -0.69, -0.69,
                                    C.byref(p)) == 1
    cnt = np.zeros(1, np.uint32)  # never dereferenced: the stream check comes first
    assert L.msv_filter_select_device(0, None, None, None, 0, -9.0, 0.7, 0.02, None, None, cnt.ctypes.data,
                                      None) == 1
    assert L.msv_vit_profile_bind_stream(None, None) == 1


@pytest.mark.parametrize("prefix", ["msv_vit", "msv_fwd"])
def test_stage_create_and_bind_validate_arguments(prefix):
    """Both stages' create refuses a transition score that is not a log-probability (positive, or NaN) before
    any device is touched, and bind_stream a NULL profile: status 1 (MSV_ERR_INVALID_ARGUMENT) from either."""
    import numpy as np
    L = _native.lib()
    create, bind = getattr(L, prefix + "_profile_create"), getattr(L, prefix + "_profile_bind_stream")
    M = 101
    msc = np.zeros((20, M), np.float32)
    tsc = np.full((M, 7), np.float32(np.log(np.float32(0.5))), np.float32)
    p = C.c_void_p()
    for bad in (0.25, np.nan):
        tsc[5, 3] = bad  # node 5, i->m
        assert create(0, msc.ctypes.data, None, tsc.ctypes.data, M, -8.0, -0.69, -0.69, C.byref(p)) == 1
        assert not p.value
    assert bind(None, None) == 1


def test_info_struct_layouts_match_the_header(tmp_path):
    """The ctypes mirrors of msv_kernel_info / msv_vit_info (hmm_fasta_viterbi_amd/_native.py) have the C header's
    field offsets and sizes (gcc on include/msv.h), and both structs keep their round-4 prefix: fields are only
    appended (a field inserted mid-struct moved `variant` for C callers built against the old header)."""
    import ctypes as C
    structs = {"msv_kernel_info": _native.KernelInfo, "msv_vit_info": _native.VitInfo}
    src = ['#include <stddef.h>', '#include <stdio.h>', '#include "msv.h"', "int main(void) {"]
    for cname, py in structs.items():
        src.append(f'  printf("{cname} size %zu\\n", sizeof({cname}));')
        for f, _ in py._fields_:
            src.append(f'  printf("{cname} {f} %zu\\n", offsetof({cname}, {f}));')
    src.append("  return 0; }")
    (tmp_path / "layout.c").write_text("\n".join(src))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", f"-I{os.path.join(ROOT, 'include')}", str(tmp_path / "layout.c"), "-o", str(exe)],
                   check=True, capture_output=True)
    got = {}
    for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines():
        s, f, v = line.split()
        got[(s, f)] = int(v)
    for cname, py in structs.items():
        assert got[(cname, "size")] == C.sizeof(py), cname
        for f, _ in py._fields_:
            assert got[(cname, f)] == getattr(py, f).offset, (cname, f)
    # the round-4 prefix of msv_vit_info: `variant` right after `device`, at byte 40
    assert got[("msv_vit_info", "variant")] == 40
    assert got[("msv_vit_info", "scratch_bytes")] > got[("msv_vit_info", "variant")]
    assert got[("msv_vit_info", "waves_per_sequence")] > got[("msv_vit_info", "scratch_bytes")]
