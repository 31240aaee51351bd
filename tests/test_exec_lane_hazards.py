"""CPU: on gfx90a and later a VALU write of EXEC (v_cmpx) must be 4 wait states ahead of v_readlane / v_readfirstlane /
v_writelane (LLVM: VALUWriteEXECRWLane).  The compiler keeps that for its own code and does not count across inline asm text,
while its register allocator puts lane accesses of its own (scalar spills) anywhere — so tools/check_dpp_hazards.py counts in the
final ISA.  Here: the checker against a listing that breaks the rule and one that keeps it, both shaped like a search level
written as a masked add (DESIGN_NOTES.md A.14); the translation units themselves: tests/test_dpp_hazards.py."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))

STEP = '''	s_mov_b64 s[20:21], exec
	v_cmpx_lt_f32 vcc, v24, v33
	v_add_u32 v22, 32, v22
	s_mov_b64 exec, s[20:21]
'''

VIOLATES = '''
_Zbad:
''' + STEP + '''	v_readfirstlane_b32 s4, v22
''' + STEP + '''	s_nop 0
	v_readlane_b32 s5, v22, 3
	v_cmpx_le_f32 vcc, v1, v2
	v_writelane_b32 v7, s5, 2
'''

KEEPS = '''
_Zgood:
''' + STEP + '''	s_nop 1
	v_readfirstlane_b32 s4, v22
''' + STEP + '''	ds_read_b32 v25, v22 offset:1032
	v_mov_b32_e32 v3, v4
	v_readlane_b32 s5, v22, 3
	v_cmpx_le_f32 vcc, v1, v2
	s_nop 3
	v_writelane_b32 v7, s5, 2
	s_mov_b64 exec, s[20:21]
	v_readlane_b32 s6, v22, 0
_Znext:
	v_readlane_b32 s7, v22, 0
'''


def test_checker_finds_lane_access_too_close_to_an_exec_write():
    import check_dpp_hazards as H
    bad = H.check(VIOLATES)
    # 2 wait states (the add, the restore), 3 (+ s_nop 0), 0
    assert sorted(ln for _, ln, _ in bad) == [7, 13, 15], bad
    assert all('EXEC' in m for _, _, m in bad)
    assert [m.split()[0] for _, _, m in sorted(bad, key=lambda b: b[1])] == ['v_readfirstlane_b32', 'v_readlane_b32', 'v_writelane_b32']


def test_checker_accepts_four_wait_states_and_scalar_exec_writes():
    import check_dpp_hazards as H
    assert H.check(KEEPS) == []
