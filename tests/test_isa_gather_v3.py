"""The hot-loop step engine (grow_spec2_kernel<16>) issues its gather from inline assembly: the loads write their
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
    assert walked >= 8  # the gather of the hot loop and of the complete step, records and flags, one block per row chunk
    assert not bad, "\n".join(bad)


def _check_by_hand(mod, tmp_path, body):
    p = tmp_path / "k.s"
    p.write_text("\n".join([mod.KERNELS[0] + "EvNS0_8SpecArgsE:", *body, ".Lfunc_end0:"]))
    return mod.check(str(p))


def test_the_check_sees_a_read_in_flight_on_one_path(tmp_path):
    """A hand-made kernel: the first read of the loaded register comes before the wait (caught), the second after it."""
    mod = _mod()
    walked, bad = _check_by_hand(mod, tmp_path, [
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
    ])
    assert walked == 1
    assert len(bad) == 1 and "v9, v8, v9" in bad[0], bad


def test_the_check_sees_a_row_register_touched_between_the_two_waits(tmp_path):
    """The two-part wait of the gather, by hand: vmcnt(N > 0) lets the record load land while the row load issued after
    it is still writing its registers -- a touch of those before the vmcnt(0) is caught, the one after it is not."""
    mod = _mod()
    walked, bad = _check_by_hand(mod, tmp_path, [
        "\t;;#ASMSTART",
        "\tglobal_load_dwordx4 v[4:7], v[0:1], off",
        "\tglobal_load_dwordx4 v[12:15], v[2:3], off",
        "\t;;#ASMEND",
        "\ts_waitcnt vmcnt(1)",
        "\tv_mov_b32_e32 v10, v5",
        "\tv_mov_b32_e32 v11, v13",
        "\ts_waitcnt vmcnt(0)",
        "\tv_mov_b32_e32 v16, v14",
        "\ts_endpgm",
    ])
    assert walked == 1
    assert len(bad) == 1 and "v11, v13" in bad[0], bad
