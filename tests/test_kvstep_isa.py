"""Audit of the decode-step kernels (arcq_kv_decode_step: kv_decode_kernel's fourth template argument) in the generated code, from one
compile of kv_cache.hip to gfx950 assembly with the product flags.  Only the kernel metadata directives are read: every decode-step
instantiation runs without a private segment, i.e. the new position's quantiser in front of a wave's last block spills nothing to
scratch.  The allocated VGPRs and the LDS of each instance are printed."""
import os
import re

import pytest

from tests.isa import HIPCC, assembly

STEP = re.compile(r"kv_decode_kernelILi0ELb[01]ELi[124]ELb1EE")        # <ARCQ_KV_INT4, bf16?, GC, STEP = true> in the mangled name

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")


@pytest.fixture(scope="module")
def metadata():
    """{mangled name: metadata directives} of every kernel in kv_cache.hip."""
    text = assembly("kv_cache.hip")
    return {m.group(1): text[m.start():text.index(".end_amdhsa_kernel", m.start())] for m in re.finditer(r"^\s*\.amdhsa_kernel (\S+)$", text, flags=re.M)}


def _int(meta, key):
    return int(re.search(r"\.amdhsa_" + key + r" (\d+)", meta).group(1))


def test_decode_step_kernels_use_no_scratch(metadata):
    step = sorted(n for n in metadata if STEP.search(n))
    assert len(step) == 6, (step, sorted(metadata))                     # fp16 / bf16 x GC in {1, 2, 4}
    for name in step:
        meta = metadata[name]
        print(f"{name}: next_free_vgpr {_int(meta, 'next_free_vgpr')}, group_segment_fixed_size {_int(meta, 'group_segment_fixed_size')}")
        assert _int(meta, "private_segment_fixed_size") == 0, f"{name}: scratch in use"
