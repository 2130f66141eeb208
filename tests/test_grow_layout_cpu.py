"""bs_grow_layout.h (sizes and scratch layout of the speculative grower's host loop), compiled for the host with
AddressSanitizer and UBSan as a stand-alone program: arithmetic only, nothing is allocated.

For n at the tile, group and wave-cap boundaries up to 2^31 - 65, K on both sides of 16, th_point_count from 0 to
10^9, and the limits of bs_selftest_grow_limits at zero and each one lowered, every region of rg_aux, rg_disp,
rg_hout and rg_geo starts at its alignment, holds at least the elements the host loop and the kernels use, overlaps
no other region and ends inside the slot; the declared aliases (pos / lmask in vmark, minr in rpos, state in dirty1,
bund in bdirty1, rcur in cand_raw, retry in dkeys_in) start with and fit into their host region; offsets stay
64-bit; no slot needs more bytes than the hand-written formula it replaces (written out again in the check); a
lowered limit changes no buffer size; and the nested structs of the misc block sit where the kernels index them."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_grow_layout_regions_aliases_and_bounds(tmp_path):
    exe = str(tmp_path / "grow_layout_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "buildingsegment_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "grow_layout_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "bad=0" in out.stdout
