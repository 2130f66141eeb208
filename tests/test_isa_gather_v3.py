"""The third step engine (grow_spec2_kernel<KC, true>) issues its gather from inline assembly: the loads write their
destination registers after the asm statement, so until an s_waitcnt covers them no instruction may read or write
those registers, on any path.  tools/check_gather_wait.py walks the generated gfx950 ISA from the first load of every
asm block; here on the default flags and on the -DBS_PROBE build (different register allocation).  No GPU needed."""
import importlib.util
import os
import shutil

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HAVE_HIPCC = shutil.which("hipcc") is not None or os.path.exists("/opt/rocm/bin/hipcc")


def _mod():
    spec = importlib.util.spec_from_file_location("check_gather_wait", os.path.join(ROOT, "tools", "check_gather_wait.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.skipif(not HAVE_HIPCC, reason="no hipcc")
@pytest.mark.parametrize("flags", [(), ("-DBS_PROBE",)], ids=["default", "probe"])
def test_no_instruction_touches_an_asm_load_before_its_wait(flags):
    mod = _mod()
    walked, bad = mod.check(mod.device_asm(list(flags)))
    assert walked >= 8  # the gather of the hot loop and of the complete step, rows and flags, for k <= 16 and k <= 32
    assert not bad, "\n".join(bad)


def test_the_check_sees_a_read_of_a_register_in_flight(tmp_path):
    """A hand-made kernel: the first read of the loaded register comes before the wait (caught), the second after it."""
    mod = _mod()
    name = mod.KERNELS[0] + "EvNS0_8SpecArgsE"
    asm = "\n".join([
        name + ":",
        "\t;;#ASMSTART",
        "\tglobal_load_dwordx4 v[4:7], v[0:1], off",
        "\tglobal_load_dword v8, v[2:3], off sc1",
        "\t;;#ASMEND",
        "\tv_add_u32_e32 v9, v8, v9",
        "\ts_cbranch_scc1 .LBB0_2",
        "\ts_waitcnt vmcnt(1)",
        "\tv_mov_b32_e32 v10, v5",
        ".LBB0_2:",
        "\ts_waitcnt vmcnt(0)",
        "\tv_mov_b32_e32 v11, v8",
        "\ts_endpgm",
        ".Lfunc_end0:",
        mod.KERNELS[1] + "EvNS0_8SpecArgsE:",
        "\ts_endpgm",
        ".Lfunc_end1:",
    ])
    p = tmp_path / "k.s"
    p.write_text(asm)
    walked, bad = mod.check(str(p))
    assert walked == 1
    assert len(bad) == 1 and "v9, v8, v9" in bad[0], bad
