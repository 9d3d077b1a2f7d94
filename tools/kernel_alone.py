#!/usr/bin/env python3
"""Compile ONE run_kernel instantiation alone to annotated ISA (seconds instead of the minutes the whole engine takes):

    python tools/kernel_alone.py "2, 1, lmc::AR1Target, 0, 1, 4" /tmp/isa/c3.s [-D...]
    python tools/isa_pair_loop.py /tmp/isa/c3.s _ZN3lmc10run_kernelILi2ELi1ENS_9AR1TargetELi0ELi1ELi4EEE

The translation unit is the library's header plus one explicit instantiation, compiled with the library's flags
(_build.HIPCC_FLAGS) and -gline-tables-only -S --cuda-device-only; the resource remarks (-Rpass-analysis=kernel-resource-usage)
go to stderr. Register allocation of a kernel compiled alone can differ by a few instructions from the same kernel inside
lmc_engine.hip."""
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from littlemcmc_amd import _build  # noqa: E402

args, out, extra = sys.argv[1], sys.argv[2], sys.argv[3:]
tu = ('#include <hip/hip_runtime.h>\n#include <cmath>\n#include "lmc_hip.h"\n#include "lmc_sampler.hpp"\n'
      "template __global__ void lmc::run_kernel<%s>(lmc::ChainArrays, lmc::SamplerParams, const double*);\n" % args)
with tempfile.TemporaryDirectory() as tmp:
    src = os.path.join(tmp, "one.hip")
    open(src, "w").write(tu)
    flags = [f for f in _build.HIPCC_FLAGS if f != "-shared"]
    cmd = [os.environ.get("HIPCC", "hipcc")] + flags + ["-gline-tables-only", "-S", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
                                                       "-I", _build.CSRC, "-I", os.path.join(ROOT, "include")] + extra + ["-o", out, src]
    sys.exit(subprocess.run(cmd).returncode)
