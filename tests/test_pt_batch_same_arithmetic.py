"""No GPU needed: pt_batch_trace_kernel must round a camera path exactly as path_trace_kernel does.

Both kernels inline the one path_trace_pixel (pt_common.hpp) and are built with contraction allowed, so which product of a sum of
products is fused and which is rounded is the compiler's choice: the back end fuses the product it finds first among the operands of an
add, and the optimiser orders those operands by where their inputs enter the kernel.  The batched kernel once read the sample's seed
beside the texel loads; the first vertex's sampled direction then had n * p.z + (t * p.x + b * p.y) listed the other way round and came
out one unit in the last place off in a few pixels per frame (tests/test_gpu_pt_batch.py sees it on the GPU).

This test holds the cause and not the symptom: in the optimised LLVM IR of the two kernels, the floating-point operations of the path,
in order, must have the same shape -- the opcode, the contract flag, and for every operand the operation that defines it, whether that is
in the same basic block (the back end fuses within a block only) and how many uses the result has (it prefers a product with one use).
Operand order is kept wherever an operand is a product, which is where it decides a fusion; elsewhere it is irrelevant and sorted.
The adaptive instantiation path_trace_kernel<true>, which an adaptive sequence runs, is held to the default one in the same way.

This rests on the compiler's habits, not on a rule of the language: a compiler upgrade may move either kernel, and this test is where
that shows first.  The remedy is then to look at where the two listings part (the assertion prints the places), not to loosen it."""
import os
import re
import subprocess

import pytest

from test_kernel_resources import FLAGS, HIPCC, ROOT

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")

ARITH = ("fmul", "fadd", "fsub", "fdiv", "fneg", "call")
MATH = ("fma", "fmuladd", "sqrt", "rcp", "rsq", "exp", "log", "maxnum", "minnum", "fabs", "floor", "rint", "ldexp", "frexp", "fract")


def optimised_ir(src):
    out = subprocess.run([HIPCC] + FLAGS + ["-emit-llvm", "-o", "-", os.path.join(ROOT, "evplp_amd", "csrc", src)], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    return out.stdout


def body_of(ir, kernel):
    lines, inside = [], False
    for line in ir.splitlines():
        if line.startswith("define") and kernel in line:
            inside = True
            continue
        if inside and line.startswith("}"):
            return lines
        if inside:
            lines.append(line)
    raise AssertionError(kernel + " is not in the unit")


def shapes(lines):
    defs, uses, block, insts = {}, {}, None, []
    for line in lines:
        m = re.match(r"^([\w.]+):", line)
        if m:
            block = m.group(1)
            continue
        m = re.match(r"^\s+(%[\w.]+) = (\w+)", line)
        rest = line
        if m:
            defs[m.group(1)] = (m.group(2), block)
            rest = line.split("=", 1)[1]
        for u in re.findall(r"%[\w.]+", rest):
            uses[u] = uses.get(u, 0) + 1
        insts.append((line, block))
    out = []
    for line, blk in insts:
        m = re.match(r"^\s+(%[\w.]+) = (?:tail )?(fmul|fadd|fsub|fdiv|fneg|call)\b(.*)", line)
        if not m:
            continue
        op = m.group(2)
        if op == "call":
            c = re.search(r"@llvm\.([\w.]+)", line)
            if not c or not any(k in c.group(1) for k in MATH):
                continue
            op = c.group(1)
        ops = []
        for u in re.findall(r"%[\w.]+", m.group(3)):
            d = defs.get(u, ("argument", None))
            if d[0] in ARITH:
                ops.append("%s%s%d" % (d[0], "=" if d[1] == blk else "^", uses.get(u, 0) if d[0] == "fmul" else 0))
            else:
                ops.append("value")                                       # a load, a phi, a select, a conversion: how it got here rounds nothing
        if op in ("fadd", "fmul") and not any(o.startswith("fmul") for o in ops):
            ops.sort()                                                    # commutative and nothing to fuse: the order changes no bit
        out.append("%s%s(%s)" % (op, " contract" if " contract " in line else "", ", ".join(ops)))
    return out


def test_the_batched_trace_contracts_as_path_trace_kernel_does():
    pt = shapes(body_of(optimised_ir("kernels_pt.hip"), "path_trace_kernelILb0E"))
    batch = shapes(body_of(optimised_ir("kernels_ptbatch.hip"), "pt_batch_trace_kernel"))
    fused = sum(1 for s in pt if s.startswith(("fadd contract", "fsub contract")) and "fmul=" in s)
    print(f"{len(pt)} floating-point operations in path_trace_kernel, {len(batch)} in pt_batch_trace_kernel; {fused} adds with a product to fuse")
    assert len(pt) > 1000 and fused > 100                                 # the comparison is of the path, not of two empty lists
    differ = [(i, a, b) for i, (a, b) in enumerate(zip(pt, batch)) if a != b]
    assert len(pt) == len(batch) and not differ, (len(pt), len(batch), differ[:6])


def test_the_adaptive_instantiation_contracts_as_the_default_one():
    """In path-trace adaptive mode the sequence runs path_trace_kernel<true>: an active tile's path there must be the default kernel's too.
    Its text begins with the retired tiles' rescale (fp64: a division and the products of the four channels); the path follows."""
    ir = optimised_ir("kernels_pt.hip")
    pt, adapt = shapes(body_of(ir, "path_trace_kernelILb0E")), shapes(body_of(ir, "path_trace_kernelILb1E"))
    head = len(adapt) - len(pt)
    print(f"{len(pt)} floating-point operations in path_trace_kernel<false>, {len(adapt)} in <true>: {adapt[:max(head, 0)]} first")
    assert head == 5 and adapt[0].startswith("fdiv") and all(s.startswith("fmul") for s in adapt[1:head]), adapt[:8]
    differ = [(i, a, b) for i, (a, b) in enumerate(zip(pt, adapt[head:])) if a != b]
    assert not differ, differ[:6]
