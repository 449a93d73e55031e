"""Blocks of 65..128 pivots: the 128-slot decision kernel (k_block_decide128: the body of k_block_chain2_t with 256
pending pivots, 32 chunks and up to four windows per ladder) and the matrix-core sweep of 128 pivots per pass
(k_sweep128_mfma with its pack kernel) as the product compiles them.  No GPU needed: the device code is compiled to
assembly and the resource lines and ladder blocks are read, as tests/test_kernel_registers.py does for the 32- and 64-slot
forms."""
import re

import pytest

from tests.test_kernel_registers import _compile_asm, _kernel_functions, _resources


@pytest.fixture(scope="module")
def device_asm(tmp_path_factory):
    return _compile_asm(tmp_path_factory, 0)


@pytest.fixture(scope="module")
def device_asm_fused(tmp_path_factory):
    return _compile_asm(tmp_path_factory, 1)


def test_decision_kernel_of_128_slots_has_no_scratch_and_a_branch_free_ladder(device_asm, device_asm_fused):
    """One instantiation per compilation, one wave per SIMD (at most 512 registers, no scratch); between an ASMSTART /
    ASMEND pair of a ladder chunk only the multiply-adds, the eight v_cmp and the s_mov of EXEC.  Four windows of eight
    chunks, straight or from a start index, in two phases: at least 128 ladder blocks."""
    for asm, fused in ((device_asm, False), (device_asm_fused, True)):
        res = _resources(asm, "k_block_decide128")
        assert len(res) == 1, sorted(res)
        for name, r in res.items():
            assert r["private_seg_size"] == 0, (name, r)
            assert r["num_vgpr"] + r["num_agpr"] <= 512, (name, r)
        for name, lines in _kernel_functions(asm, "k_block_decide128").items():
            blocks, cur = [], None
            for ln in lines:
                if ln.startswith(";;#ASMSTART"):
                    cur = []
                elif ln.startswith(";;#ASMEND"):
                    if cur is not None:
                        blocks.append(cur)
                    cur = None
                elif cur is not None and ln:
                    cur.append(ln)
            arith = ("v_fma_f64",) if fused else ("v_mul_f64", "v_add_f64")
            ladders = [b for b in blocks if sum(1 for ln in b if ln.startswith(arith)) == (8 if fused else 16)]
            assert len(ladders) >= 128, (name, len(ladders))
            for b in ladders:
                assert all(ln.startswith(arith + ("v_cmp_ge_i32", "s_mov_b64")) for ln in b), (name, b)
            masked = [b for b in ladders if any(ln.startswith("v_cmp_ge_i32") for ln in b)]
            assert masked and all(sum(1 for ln in b if ln.startswith("v_cmp_ge_i32")) == 8 and
                                  b[0] == "s_mov_b64 %s, exec" % b[0].split()[1].rstrip(",") and
                                  b[-1].startswith("s_mov_b64 exec, ") for b in masked), name


def test_sweep_of_128_pivots_is_in_the_fused_compilation_only(device_asm, device_asm_fused):
    """The product's fused compilation instantiates k_sweep128_mfma (<NT, OOP>: four) and k_pack_multipliers_mfma128, two
    workgroups per CU (no scratch, at most 256 registers); the default compilation has neither."""
    res = _resources(device_asm_fused, "k_sweep128_mfma")
    assert len(res) == 4, sorted(res)
    for name, r in res.items():
        assert r["private_seg_size"] == 0 and r["num_vgpr"] + r["num_agpr"] <= 256, (name, r)
    assert re.search(r"\.amdhsa_kernel \S*k_pack_multipliers_mfma128", device_asm_fused)
    for k in ("k_sweep128_mfma", "k_pack_multipliers_mfma128"):
        assert not re.search(r"\.amdhsa_kernel \S*%s" % k, device_asm), k
