"""No GPU needed: what the VPL gather with entry cuts -- gather_vpl_kernel<true, ...>, default, calibration (COST) and adaptive (ADAPT)
variant -- relies on once the VPL's record travels through the cut ring (kernels_gather.hip, EVPLP_VPL_RING):

  * LDS: the kernel's static ring (3 buffers of 256 + 96 bytes) plus the dynamic size its launcher asks for at k = 2 splits per wavefront
    stay within 5120 bytes, the most a single-wavefront workgroup may use for eight waves per SIMD;
  * zero scratch;
  * no scalar fetch of the record array in the per-VPL loop: the record is read from the ring buffer.

The scalar record fetches are the statements of sload8 / sload16 (device_common.hpp): one s_load_dwordx8 or s_load_dwordx16 and its wait, in a
statement of their own.  The walks from the root -- gather_vpl_kernel<false, ...>, untouched -- keep them: head in front of the walk, head and
tail behind it.  That is the positive control of the detector below."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "evplp_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-munsafe-fp-atomics", "-fno-slp-vectorize", "-S", "--cuda-device-only", "-w"]
LDS_PER_WAVE = 5120                      # 160 KB per CU / 32 single-wavefront workgroups
VARIANTS = {"default": "ILb%dELb0ELb0E", "COST": "ILb%dELb1ELb0E", "ADAPT": "ILb%dELb0ELb1E"}

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")


@pytest.fixture(scope="module")
def listing():
    out = subprocess.run([HIPCC] + FLAGS + ["-o", "-", os.path.join(CSRC, "kernels_gather.hip")], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    return out.stdout


def kernel_name(listing, cut, variant):
    names = set(re.findall(r"^(_ZN5evplp17gather_vpl_kernel" + VARIANTS[variant] % cut + r"\w*):", listing, re.M))
    assert len(names) == 1, (cut, variant, names)
    return names.pop()


def metadata(listing, name):
    """the fields of the kernel's block in amdhsa.kernels"""
    blocks = re.split(r"^  - \.agpr_count:", listing[listing.index("amdhsa.kernels:"):], flags=re.M)
    mine = [b for b in blocks if re.search(r"^\s+\.name:\s+" + re.escape(name) + r"\s*$", b, re.M)]
    assert len(mine) == 1, name
    return {k: int(v) for k, v in re.findall(r"^\s+\.(group_segment_fixed_size|private_segment_fixed_size|vgpr_spill_count|vgpr_count|sgpr_count):\s+(\d+)", mine[0], re.M)}


def asm_statements(listing, name):
    """the inline-asm statements of the kernel's body: a list of instruction lists"""
    body = listing[re.search(r"^" + re.escape(name) + r":", listing, re.M).start():]
    body = body[:body.index(".Lfunc_end")]
    out = []
    for block in re.findall(r";;#ASMSTART\n(.*?);;#ASMEND", body, re.S):
        out.append([l.strip() for l in block.splitlines() if l.strip() and not l.strip().startswith(";")])
    return out


def is_record_fetch(stmt):
    """sload8 / sload16 / sload16x2: wide scalar loads and one wait, nothing else"""
    ops = [l.split()[0] for l in stmt]
    return len(ops) >= 2 and ops[-1] == "s_waitcnt" and all(o in ("s_load_dwordx8", "s_load_dwordx16") for o in ops[:-1])


def launcher_dynamic_lds(tmp_path, ks):
    """gather_vpl_lds_bytes(k) of kernels.h -- the expression launch_gather_vpl_items passes as the dynamic LDS size -- evaluated by a host program"""
    src = tmp_path / "lds.cpp"
    src.write_text('#include <cstdio>\n#include "kernels.h"\nint main() { ' + " ".join('std::printf("%%zu\\n", evplp::gather_vpl_lds_bytes(%d));' % k for k in ks) + " return 0; }\n")
    exe = tmp_path / "lds"
    cc = subprocess.run([HIPCC, "-O1", "-std=c++17", "-x", "c++", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I" + CSRC, "-I" + os.path.join(ROOT, "include"),
                         str(src), "-o", str(exe)], capture_output=True, text=True, timeout=300)
    assert cc.returncode == 0, cc.stderr[-2000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0
    return dict(zip(ks, (int(x) for x in run.stdout.split())))


def test_launcher_calls_the_size_the_test_evaluates():
    text = open(os.path.join(CSRC, "kernels_gather.hip")).read()
    body = text[text.index("void launch_gather_vpl_items("):]
    body = body[:body.index("\n}\n")]
    assert "const size_t lds = gather_vpl_lds_bytes(a.splits_per_wave);" in body
    assert body.count("dim3(64), lds, s, a, ad)") == 6, "every variant of the kernel is launched with that size"


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_ring_kernels_fit_eight_waves_and_fetch_no_record(listing, tmp_path, variant):
    name = kernel_name(listing, 1, variant)
    md = metadata(listing, name)
    dyn = launcher_dynamic_lds(tmp_path, (1, 2))
    ring = 3 * (256 + 96)
    print(f"\n{variant}: static LDS {md['group_segment_fixed_size']} B, dynamic at k = 1 / 2 {dyn[1]} / {dyn[2]} B, {md['vgpr_count']} VGPRs, {md['sgpr_count']} SGPRs")
    assert md["group_segment_fixed_size"] == ring, md                     # slot + record per buffer, three buffers
    assert dyn[2] == (640 + 192) * 4 and dyn[1] == 640 * 4, dyn           # pixel data + log2 k fold levels (none at k = 1)
    assert md["group_segment_fixed_size"] + dyn[2] <= LDS_PER_WAVE, (md, dyn)
    assert md["private_segment_fixed_size"] == 0 and md["vgpr_spill_count"] == 0, md
    assert md["vgpr_count"] <= 64 and md["sgpr_count"] < 81, md
    stmts = asm_statements(listing, name)
    fetches = [s for s in stmts if is_record_fetch(s)]
    assert not fetches, fetches
    # ... the record comes from the ring buffer: five LDS reads issued together with the kernel arguments' two scalar loads, one wait
    tails = [s for s in stmts if any(l.startswith("ds_read_b128") for l in s) and any(l.startswith("s_load_dwordx4") for l in s)]
    assert len(tails) == 1, tails
    ops = [l.split()[0] for l in tails[0]]
    assert ops.count("ds_read_b128") + ops.count("ds_read_b96") == 5 and ops.count("s_waitcnt") == 1 and ops[-1] == "s_waitcnt", tails[0]
    # ... and one DMA instruction per step moves slot and record (two more fill the ring in front of the loop)
    assert sum(1 for s in stmts for l in s if l.startswith("global_load_lds_dwordx4")) == 3


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_walks_from_the_root_keep_their_scalar_record_fetches(listing, variant):
    """the positive control: the detector finds the fetches where they are -- head, then head and tail again behind the walk"""
    name = kernel_name(listing, 0, variant)
    stmts = asm_statements(listing, name)
    fetches = [[l.split()[0] for l in s[:-1]] for s in stmts if is_record_fetch(s)]
    assert fetches.count(["s_load_dwordx8"]) == 2 and fetches.count(["s_load_dwordx16"]) == 1, fetches
    assert not any(l.startswith("global_load_lds") for s in stmts for l in s)
    assert metadata(listing, name)["group_segment_fixed_size"] == 0
