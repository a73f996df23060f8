"""Build-time pin of DESIGN.md §3's resource claim for TGCN's one-launch recurrence (csrc/temporal.hip): all sixteen instances
tgcn_fwd_kernel<NT> / tgcn_bwd_kernel<NT>, NT = 1 .. 8, exist in the gfx950 code object, none uses scratch (private_segment_fixed_size 0,
vgpr_spill_count 0), and each fits the 512 registers (VGPR + AGPR) a wave of a 256-thread block can have.  tg_prod's scheduling fence is
what keeps this true from NT = 5 on; a change that lets the fragment reads be hoisted again shows here, without a GPU.

Reads the code object's notes (the AMDGPU metadata the loader itself uses) — no disassembly."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBJDIR = os.path.join(ROOT, "graphneuralnetworks.jl_amd", "lib", "obj")
OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"
READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"
NTS = tuple(range(1, 9))


def kernel_notes(obj_name, tmp_path):
    """{mangled kernel name: {key: value text}} from the amdhsa.kernels metadata of the gfx950 code object bundled in lib/obj/<obj_name>"""
    src = os.path.join(OBJDIR, obj_name)
    if not os.path.exists(src):
        import __graft_entry__ as ge
        ge.build()
    obj = os.path.join(tmp_path, obj_name)
    shutil.copy(src, obj)
    subprocess.check_call([OBJDUMP, "--offloading", obj], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    code = [f for f in os.listdir(tmp_path) if f.startswith(obj_name + ".") and "amdgcn" in f]
    assert len(code) == 1 and code[0].endswith("gfx950"), f"expected one gfx950 code object in {obj_name}, found {code}"
    text = subprocess.check_output([READELF, "--notes", os.path.join(tmp_path, code[0])], text=True)
    kernels, cur = {}, None
    for line in text.splitlines():
        m = re.match(r"^  (- | {2})\.(\w+):\s*(.*)$", line)          # an entry of amdhsa.kernels (its .args entries sit deeper)
        if not m:
            continue
        if m.group(1) == "- ":
            cur = {}
        if cur is not None:
            cur[m.group(2)] = m.group(3).strip().strip("'")
            if m.group(2) == "name":
                kernels[cur["name"]] = cur
    return kernels


def tgcn_instances(kernels):
    """{('fwd' | 'bwd', NT): notes}"""
    out = {}
    for name, notes in kernels.items():
        m = re.search(r"\d+tgcn_(fwd|bwd)_kernelILi(\d+)EE", name)
        if m:
            key = (m.group(1), int(m.group(2)))
            assert key not in out, f"two code objects for {key}"
            out[key] = notes
    return out


@pytest.mark.skipif(not (os.path.exists(OBJDUMP) and os.path.exists(READELF)), reason="no llvm-objdump / llvm-readelf in this image")
def test_all_sixteen_recurrence_instances_fit_the_register_file_without_scratch(tmp_path):
    inst = tgcn_instances(kernel_notes("temporal.o", str(tmp_path)))
    assert sorted(inst) == sorted((d, nt) for d in ("fwd", "bwd") for nt in NTS), sorted(inst)
    figures = {}
    for key in sorted(inst):
        n = inst[key]
        vgpr, agpr = int(n["vgpr_count"]), int(n["agpr_count"])
        figures[key] = (vgpr, agpr)
        assert int(n["private_segment_fixed_size"]) == 0, f"tgcn_{key[0]}_kernel<{key[1]}> uses {n['private_segment_fixed_size']} bytes of scratch"
        assert int(n["vgpr_spill_count"]) == 0, f"tgcn_{key[0]}_kernel<{key[1]}> spills {n['vgpr_spill_count']} registers"
        assert vgpr <= 512, f"tgcn_{key[0]}_kernel<{key[1]}>: vgpr_count {vgpr}"
        assert agpr <= vgpr
    print("(vgpr_count, agpr_count):", figures)
