"""The host side of the MazeWorld fused rollouts (no GPU): the argument checks of xv_maze_rollout / xv_maze_rollout_agent,
the host restatement of the exploration draws against the oracle's Philox, and the header additions as plain C."""
import ctypes as C
import os
import subprocess

import pytest

from xenoverse_amd import _lib
from xenoverse_amd.mazeworld.rollout import RECORD, TEACHER, _RolloutOut

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _autoreset():
    from xenoverse_amd.engine import AUTORESET
    return AUTORESET["same_step"], AUTORESET["next_step"], AUTORESET["disabled"]


def _out(frames=False, final_frames=False, final_pose=False, teacher=False, drop=()):
    """an xv_maze_rollout_out whose pointers are never followed (the check is host code)"""
    buf = C.create_string_buffer(64)
    p = C.addressof(buf)
    names = [f[0] for f in RECORD] + (["final_pose"] if final_pose else []) + (["frames"] if frames else []) + \
        (["final_frames"] if final_frames else []) + ([f[0] for f in TEACHER] if teacher else [])
    o = _RolloutOut(**{k: p for k in names if k not in drop})
    o._keep = buf
    return o


def _check(n_env=8, mode=1, auto=None, T=16, stride=0, actions=True, out=None, agent=0, eps=0.0):
    lib = _lib.load()
    same = _autoreset()[0]
    buf = C.create_string_buffer(8)
    return lib.xv_maze_rollout_check(n_env, mode, same if auto is None else auto, T, stride,
                                     C.addressof(buf) if actions else None, None if out is None else C.byref(out), agent, eps)


def test_rollout_check_accepts_good_argument_sets():
    same, nxt, dis = _autoreset()
    assert _check(out=_out()) == 0
    assert _check(out=_out(final_pose=True)) == 0
    for auto in (same, nxt, dis):
        for mode in (0, 1, 2):
            assert _check(mode=mode, auto=auto, out=_out()) == 0
    assert _check(stride=1, out=_out(frames=True)) == 0
    assert _check(stride=4, out=_out(frames=True, final_frames=True, final_pose=True)) == 0
    assert _check(T=3, stride=4, out=_out()) == 0                       # T // s == 0: nothing is painted
    assert _check(T=1, out=_out()) == 0
    assert _check(actions=False, agent=1, eps=0.0, out=_out(teacher=True)) == 0
    assert _check(actions=False, agent=1, eps=1.0, mode=2, stride=2, out=_out(teacher=True, frames=True)) == 0


def test_rollout_check_refuses_each_bad_argument():
    same, nxt, dis = _autoreset()
    bad = [dict(out=None), dict(n_env=0, out=_out()), dict(T=0, out=_out()), dict(T=-1, out=_out()),
           dict(stride=-1, out=_out()), dict(mode=3, out=_out()), dict(mode=-1, out=_out()), dict(auto=3, out=_out()),
           dict(actions=False, out=_out()),
           dict(stride=1, out=_out()),                                   # painted steps, no frames
           dict(stride=0, out=_out(frames=True)),                        # frames, nothing painted
           dict(T=3, stride=4, out=_out(frames=True)),
           dict(stride=0, out=_out(final_frames=True)),
           dict(stride=1, auto=nxt, out=_out(frames=True, final_frames=True)),
           dict(auto=dis, out=_out(final_pose=True)),
           # the agent call: given actions, a Continuous space, another autoreset mode, epsilon out of range, missing outputs
           dict(agent=1, out=_out(teacher=True)),
           dict(actions=False, agent=1, mode=0, out=_out(teacher=True)),
           dict(actions=False, agent=1, auto=nxt, out=_out(teacher=True)),
           dict(actions=False, agent=1, eps=-0.1, out=_out(teacher=True)),
           dict(actions=False, agent=1, eps=1.5, out=_out(teacher=True)),
           dict(actions=False, agent=1, eps=float("nan"), out=_out(teacher=True)),
           dict(actions=False, agent=1, out=_out())]
    bad += [dict(out=_out(drop=(f[0],))) for f in RECORD]
    bad += [dict(actions=False, agent=1, out=_out(teacher=True, drop=(f[0],))) for f in TEACHER]
    for kw in bad:
        assert _check(**kw) != 0, kw
        assert b"xv_maze_rollout_check" in _lib.load().xv_last_error()


def test_rollout_struct_matches_the_header():
    """the ctypes mirror of xv_maze_rollout_out has the header's members in the header's order"""
    import re
    txt = open(os.path.join(ROOT, "include", "xeno.h")).read()
    body = re.search(r"typedef struct xv_maze_rollout_out \{(.*?)\} xv_maze_rollout_out;", txt, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    members = re.findall(r"\*\s*([a-z_]+)\s*;", body)
    assert members == [k for k, _ in _RolloutOut._fields_]


def test_header_additions_compile_as_plain_c(tmp_path):
    src = tmp_path / "r.c"
    src.write_text('#include "xeno.h"\n'
                   'int main(void) {\n'
                   '  xv_maze_rollout_out o = {0};\n'
                   '  int (*a)(xv_maze*, const void*, int, int, int, int, const xv_maze_rollout_out*) = xv_maze_rollout;\n'
                   '  int (*b)(xv_maze_agent*, xv_maze_agent*, int, double, int, const xv_maze_rollout_out*) = xv_maze_rollout_agent;\n'
                   '  int (*c)(int, int, int, int, int, const void*, const xv_maze_rollout_out*, int, double) = xv_maze_rollout_check;\n'
                   '  return (o.reward == 0 && a != 0 && b != 0 && c != 0) ? 0 : 1;\n'
                   '}\n')
    obj = str(tmp_path / "r.o")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-c", str(src), "-o", obj])
