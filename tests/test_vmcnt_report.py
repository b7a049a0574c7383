"""tools/vmcnt_report.py on a small canned listing: the token sequence of every loop, the steady-state wait and what the back
edge carries (a loop that drains its own prefetch shows a small vmcnt behind its last memory operation)."""
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LISTING = """\t.text
\t.globl\t_ZN4dcmt5k_oneILb1EEEvPKf
_ZN4dcmt5k_oneILb1EEEvPKf:              ; @_ZN4dcmt5k_oneILb1EEEvPKf
; %bb.0:
\ts_load_dwordx4 s[0:3], s[4:5], 0x0
\tbuffer_load_ushort v1, v0, s[0:3], 0 offen
\ts_waitcnt vmcnt(0) lgkmcnt(0)
.LBB0_1:                                ; =>This Loop Header: Depth=1
\tbuffer_load_ushort v2, v0, s[0:3], 0 offen
\tbuffer_load_dword v3, v0, s[0:3], s6 offen
\ts_waitcnt vmcnt(5)
\tv_add_u32_e32 v4, v1, v2
\ts_cbranch_scc1 .LBB0_3
; %bb.2:
\tv_mov_b32_e32 v4, 0
.LBB0_3:                                ;   in Loop: Header=BB0_1
\tbuffer_store_dwordx2 v[4:5], v0, s[0:3], 0 offen
\ts_waitcnt lgkmcnt(0)
\ts_waitcnt vmcnt(1)
\tv_lshl_or_b32 v1, v3, 16, v2
\ts_waitcnt vmcnt(0)
\ts_cbranch_vccnz .LBB0_1
; %bb.4:
\ts_endpgm
.Lfunc_end0:
\t.globl\t_ZN4dcmt5k_twoEvPf
_ZN4dcmt5k_twoEvPf:                     ; @_ZN4dcmt5k_twoEvPf
.LBB1_1:
\tglobal_load_dword v1, v0, s[0:1]
\ts_waitcnt vmcnt(7)
\tv_add_f32_e32 v2, v1, v1
\tglobal_store_dword v0, v2, s[2:3]
\tglobal_atomic_add_u32 v0, v2, s[2:3]
\ts_branch .LBB1_1
.Lfunc_end1:
"""


def _tool():
    spec = importlib.util.spec_from_file_location("vmcnt_report", os.path.join(ROOT, "tools", "vmcnt_report.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_draining_loop_is_reported_with_its_back_edge_wait():
    t = _tool()
    name, lines = t.function_body(LISTING, "k_one")
    assert name == "_ZN4dcmt5k_oneILb1EEEvPKf"
    (lp,) = t.loops(lines)
    assert lp["label"] == ".LBB0_1"
    assert lp["tokens"] == ["L", "L", "w5", "|", "S", "w1", "w0"]     # the load and the wait ahead of the loop are not part of it
    assert lp["steady"] == 5 and lp["back_edge"] == 0
    assert lp["valu"] == 3 and lp["branches"] == 2 and lp["inner"] == 0


def test_loop_without_a_wait_behind_its_last_operation():
    t = _tool()
    (lp,) = t.loops(t.function_body(LISTING, "k_two")[1])
    assert lp["tokens"] == ["L", "w7", "S", "A"]
    assert lp["steady"] == 7 and lp["back_edge"] is None


def test_report_text_and_unknown_kernel():
    t = _tool()
    text = t.report(LISTING, "k_one")
    assert text.splitlines()[0] == "_ZN4dcmt5k_oneILb1EEEvPKf"
    assert "steady vmcnt 5  back edge vmcnt 0" in text and "L L w5 | S w1 w0" in text
    assert t.report(LISTING, "k_one", min_ops=4).count("\\n") == 0     # filtered out: three operations
    try:
        t.function_body(LISTING, "k_three")
    except KeyError:
        pass
    else:
        raise AssertionError("a missing kernel must be an error")
