"""The member table behind the scratch guard (bs_selftest_scratch_*, csrc/bs_capi.hip) lists every DevBuf / HostBuf of
bs_ctx: the library counts the buffers a context constructs against it, which needs no device, and the source of
bs_common.h is counted here a second way.  A buffer added to bs_ctx and not listed fails both (and every bs_create)."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared_buffers():
    """(name, count) of every bs::DevBuf / bs::HostBuf member the source of struct bs_ctx declares."""
    txt = open(os.path.join(ROOT, "buildingsegment_amd", "csrc", "bs_common.h")).read()
    body = txt[txt.index("struct bs_ctx : bs_ctx_handles {"):]
    body = body[:body.index("\n};")]
    body = re.sub(r"//[^\n]*", "", body)
    enums = dict(BT_COUNT=len(re.search(r"enum \{ (BT_OFF.*?), BT_COUNT \}", txt).group(1).split(",")))
    out = []
    for decl in re.findall(r"bs::(?:DevBuf|HostBuf)\s+([^;]+);", body):
        for item in decl.split(","):
            m = re.fullmatch(r"\s*(\w+)(?:\[([\w:]+)\])?\s*", item)
            assert m, item
            dim = m.group(2)
            out.append((m.group(1), 1 if dim is None else int(enums.get(dim.split("::")[-1], dim))))
    return out


def test_member_table_lists_every_buffer_of_the_context():
    from buildingsegment_amd import _lib, build
    build.build()
    L = _lib.load()
    n = C.c_int64(0)
    assert L.bs_selftest_scratch_list(None, None, 0, C.byref(n)) == 0, "bs_ctx has a buffer the member table omits"
    decl = _declared_buffers()
    assert len(set(k for k, _ in decl)) == len(decl)
    assert n.value == sum(c for _, c in decl) and n.value > 400
    # every declared member is named in the table, as a single buffer or as an array
    src = open(os.path.join(ROOT, "buildingsegment_amd", "csrc", "bs_capi.hip")).read()
    table = src[src.index("void scratch_members("):src.index("#undef BS_ONE")]
    for name, count in decl:
        if name == "rg_hout":
            assert '"rg_hout"' in table
        else:
            assert re.search(r"BS_%s\(%s\)" % ("ONE" if count == 1 and name != "bt" else "ARR", name), table), name


def test_slot_structs_mirror_the_header():
    from buildingsegment_amd import _lib
    assert C.sizeof(_lib.ScratchSlot) == 24 + 8 * 5 + 8
    assert C.sizeof(_lib.ScratchReport) == 32 + 8 * C.sizeof(_lib.ScratchSlot)
    txt = open(os.path.join(ROOT, "include", "bs_api.h")).read()
    assert "#define BS_SCRATCH_REPORT_MAX 8" in txt and "char name[24];" in txt
