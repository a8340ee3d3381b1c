"""GPU: the argument checks of the training backwards.  Each of the twelve C entries pp_{unit,down,neck}_backward{,_affine,_bn,_mp}
and the three pp_*_backward_path entries is called through ctypes with valid small arguments but for one fault, and must refuse it with
PP_E_ARG and a message that starts with the entry's prefix and names the fault.  The _mp entries are called in mode 1, whose tensor
faults pp_unit_backward_mp reports under "pp_unit_backward:" (the strided stage and the upsampler use their own names); the _path
entries report shape faults under the prefix of the _mp entry they answer for.  No call gets past its checks, so no kernel is launched."""
import ctypes

import pytest
import torch

from conftest import load_pkg
from train_common import small_cfg

pytestmark = pytest.mark.gpu
PP_E_ARG = 1
NB = 2
_STATE = {}

# the parameters of every entry in ABI order (ctx first and implied); lower-case words are looked up in the family's values
UNIT_SPEC = {
    "pp_unit_backward": "C h w u wgt dy dskip nb dw du stream",
    "pp_unit_backward_affine": "C h w u wgt scale shift dy dskip nb dw du dscale dshift stream",
    "pp_unit_backward_bn": "C h w u wgt scale shift mean var dy dskip nb dw du dscale dshift chunk_frames stream",
    "pp_unit_backward_mp": "mode C h w u wgt dy dskip nb dw du stream",
    "pp_unit_backward_path": "mode C h w",
}
DOWN_SPEC = {
    "pp_down_backward": "cin cout hin win x wgt z dy nb dw dx stream",
    "pp_down_backward_affine": "cin cout hin win x wgt z scale shift dy nb dw dx dscale dshift stream",
    "pp_down_backward_bn": "cin cout hin win x wgt z scale shift mean var dy nb dw dx dscale dshift chunk_frames stream",
    "pp_down_backward_mp": "mode cin cout hin win x wgt z dy nb dw dx stream",
    "pp_down_backward_path": "mode cin cout hin win",
}
NECK_SPEC = {
    "pp_neck_backward": "branch x wgt y dy nb dw dx stream",
    "pp_neck_backward_affine": "branch x wgt scale shift y dy nb dw dx dscale dshift stream",
    "pp_neck_backward_bn": "branch x wgt scale shift mean var y dy nb dw dx dscale dshift chunk_frames stream",
    "pp_neck_backward_mp": "mode branch x wgt y dy nb dw dx stream",
    "pp_neck_backward_path": "mode branch",
}
SPEC = {**UNIT_SPEC, **DOWN_SPEC, **NECK_SPEC}

# fault -> (the arguments it replaces, per family where they differ (None: the family has no such fault; "+n": the pointer moved by n
# bytes), the phrase the message must contain).  An entry takes part in a fault when it has every argument the fault names.
FAULTS = {
    "nb": ({"nb": 0}, "nb must be"),
    "null_dy": ({"dy": None}, "null pointer"),
    "w_offset": ({"wgt": "+4"}, "16-byte aligned"),
    "illegal": ({"unit": {"C": 96}, "down": {"cout": 96}, "neck": {"branch": 3}}, " must be "),
    "one_element": ({"unit": {"h": 1, "w": 1}, "down": {"hin": 1, "win": 1}, "neck": None}, ">= 2"),
    "dscale_alone": ({"dshift": None}, "go together"),
    "need_du": ({"unit": {"du": None, "dscale": "+0"}, "down": None, "neck": None}, "need du"),  # "+0": as it is, but the entry must have it
    "dscale_offset": ({"dscale": "+4"}, "8-byte"),
    "chunk_frames": ({"chunk_frames": -1}, "chunk_frames must be >= 0"),
    "mode": ({"mode": 3}, "mode must be"),
}


def family_of(entry):
    return entry.split("_")[1]


def applies(entry, fault):
    """Whether the entry has the argument(s) the fault replaces."""
    change = FAULTS[fault][0]
    change = change.get(family_of(entry), None) if set(change) <= {"unit", "down", "neck"} else change
    return change is not None and set(change) <= set(SPEC[entry].split())


def prefix(entry, fault):
    if fault == "mode":
        return entry + ":"
    if entry in ("pp_unit_backward_mp", "pp_unit_backward_path"):
        return "pp_unit_backward:"
    return entry.replace("_path", "_mp") + ":"


def state():
    """The engine (BEV 16 x 8, max_batch 2, no weights: the entries are stateless) and valid arguments of every family."""
    if not _STATE:
        load_pkg().install()
        eng = load_pkg("engine").Engine(small_cfg(32, 16, NB))
        assert (eng.H, eng.W, eng.max_batch) == (16, 8, NB)
        f32 = lambda *s: torch.zeros(*s, dtype=torch.float32, device="cuda")  # noqa: E731
        f64 = lambda n: torch.zeros(n + 1, dtype=torch.float64, device="cuda")  # noqa: E731  one element of slack: an entry is offset by 4 bytes
        common = {"mode": 1, "nb": NB, "chunk_frames": 0, "stream": None}
        C, h, w = 64, 3, 2
        unit = dict(common, C=C, h=h, w=w, u=f32(NB, C, h, w), wgt=f32(C * C * 9 + 4), dy=f32(NB, C, h, w), dskip=f32(NB, C, h, w), dw=f32(C, C, 3, 3),
                    du=f32(NB, C, h, w))
        cin, cout, hin, win = 64, 64, 3, 4
        down = dict(common, cin=cin, cout=cout, hin=hin, win=win, x=f32(NB, cin, hin, win), wgt=f32(cout * cin * 9 + 4), z=f32(NB, cout, 2, 2),
                    dy=f32(NB, cout, 2, 2), dw=f32(cout, cin, 3, 3), dx=f32(NB, cin, hin, win))
        neck = dict(common, branch=0, x=f32(NB, 64, 16, 8), wgt=f32(64 * 64 + 4), y=f32(NB, 320, 16, 8), dy=f32(NB, 320, 16, 8), dw=f32(64, 64, 1, 1),
                    dx=f32(NB, 64, 16, 8))
        for fam in (unit, down, neck):
            fam.update(scale=f32(64), shift=f32(64), mean=f32(64), var=f32(64), dscale=f64(64), dshift=f64(64))
        _STATE.update(eng=eng, unit=unit, down=down, neck=neck)
    return _STATE


def raw(v):
    """A value of the tables as a ctypes argument."""
    return ctypes.c_void_p(v.data_ptr()) if isinstance(v, torch.Tensor) else v


def refused(eng, entry, vals, fault):
    """Calls `entry` with the family's values `vals` changed by `fault` -> (return code, message)."""
    change = FAULTS[fault][0]
    change = change[family_of(entry)] if set(change) <= {"unit", "down", "neck"} else change
    vals = dict(vals)
    for k, v in change.items():
        vals[k] = ctypes.c_void_p(vals[k].data_ptr() + int(v)) if isinstance(v, str) else v
    rc = getattr(eng.lib, entry)(eng.ctx, *[raw(vals[k]) for k in SPEC[entry].split()])
    if entry.endswith("_path"):
        rc = -rc  # the modes are 0 .. 2, so the path entries return an error as the negated code
    return rc, eng.lib.pp_last_error(eng.ctx).decode()


PAIRS = [(e, f) for e in SPEC for f in FAULTS if applies(e, f)]


def test_the_table_covers_the_entries():
    by_fault = {f: {e for e, g in PAIRS if g == f} for f in FAULTS}
    runs = {e for e in SPEC if not e.endswith("_path")}
    assert len(runs) == 12 and by_fault["nb"] == by_fault["null_dy"] == by_fault["w_offset"] == runs
    assert by_fault["illegal"] == set(SPEC)
    assert by_fault["one_element"] == set(UNIT_SPEC) | set(DOWN_SPEC)
    affine = {e for e in runs if e.endswith(("_affine", "_bn"))}
    assert by_fault["dscale_alone"] == by_fault["dscale_offset"] == affine and len(affine) == 6
    assert by_fault["need_du"] == {"pp_unit_backward_affine", "pp_unit_backward_bn"}
    assert by_fault["chunk_frames"] == {e for e in runs if e.endswith("_bn")}
    assert by_fault["mode"] == {e for e in SPEC if e.endswith(("_mp", "_path"))}


@pytest.mark.parametrize("entry,fault", PAIRS, ids=[f"{e}-{f}" for e, f in PAIRS])
def test_fault_is_refused(entry, fault):
    st = state()
    rc, msg = refused(st["eng"], entry, st[family_of(entry)], fault)
    print(f"{entry}, {fault}: rc {rc}, {msg!r}")
    assert rc == PP_E_ARG, (rc, msg)
    assert msg.startswith(prefix(entry, fault)), msg
    assert FAULTS[fault][1] in msg, msg
