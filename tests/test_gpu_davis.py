"""The DAVIS -> ADDER chain on the device (include/adder_davis.h, adder_amd.davis) against davis_oracle: events byte for
byte and the camera state planes after every packet (last ln as bit patterns), the refusals, the mirror's switch and
the file tool."""
import ctypes as C

import numpy as np
import pytest

import adder_amd as A
import davis_cases as DC
import davis_oracle as DO
from adder_amd import davis as D

pytestmark = pytest.mark.gpu

ALL = DC.CASES + DC.SEEDED
BY_NAME = {c["name"]: c for c in ALL}
_oracle = {}


def oracle(name):
    """(push results, finish events, all events) of a case: computed once, read only."""
    if name not in _oracle:
        c = BY_NAME[name]
        _oracle[name] = DO.run(c["packets"], c["W"], c["H"], c["mode"], tps=c["tps"], ref_time=c["ref_time"], dtm=c["dtm"],
                               crf=c["crf"])
    return _oracle[name]


def make(case, **over):
    kw = dict(width=case["W"], height=case["H"], mode=case["mode"], tps=case["tps"], ref_time=case["ref_time"],
              delta_t_max=case["dtm"], crf=case["crf"])
    kw.update(over)
    return D.HipDavis(**kw)


def push(dv, pk, **kw):
    return dv.push(np.asarray(pk["frame"], np.float64), float(pk["c"]), int(pk["start"]), int(pk["end"]), pk["before"],
                   pk["after"], has_events=dv.mode != D.FRAMED, **kw)


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def check_state(dv, want):
    ts, ln = dv.pixel_state()
    assert np.array_equal(ts, want["last_ts"])
    assert np.array_equal(bits(ln), bits(want["last_ln"]))


@pytest.mark.parametrize("name", [c["name"] for c in ALL])
def test_events_and_state_equal_the_oracle(name):
    case = BY_NAME[name]
    res, fin, _ = oracle(name)
    dv = make(case)
    for pk, want in zip(case["packets"], res):
        got = push(dv, pk)
        assert len(got) == len(want["events"]) and got.tobytes() == want["events"].tobytes()
        assert dv.last_frame_events() == want["frame_events"]
        check_state(dv, want)
    got = dv.finish()
    assert len(got) == len(fin) and got.tobytes() == fin.tobytes()
    dv.close()


def _device_events(ev, torch):
    ev = np.ascontiguousarray(ev, D.DAVIS_EVENT_DTYPE)
    return torch.from_numpy(ev.view(np.uint8).reshape(-1).copy()).cuda() if len(ev) else None


@pytest.mark.parametrize("name", ["seeded_mode1", "seeded_mode0", "counts"])
def test_device_and_host_push_forms_agree(name):
    import torch
    case = BY_NAME[name]
    res = oracle(name)[0]
    dv = make(case)
    for pk, want in zip(case["packets"], res):
        frame = torch.from_numpy(np.ascontiguousarray(pk["frame"], np.float64)).cuda()
        out = dv.push(frame, float(pk["c"]), int(pk["start"]), int(pk["end"]), _device_events(pk["before"], torch),
                      _device_events(pk["after"], torch), has_events=case["mode"] != D.FRAMED,
                      stream=torch.cuda.current_stream().cuda_stream)
        assert out.cpu().numpy().tobytes() == want["events"].tobytes()
        check_state(dv, want)
    dv.close()


def _twin(case, upto):
    """A context that has taken packets [0, upto) and nothing else."""
    dv = make(case)
    for pk in case["packets"][:upto]:
        push(dv, pk)
    return dv


def _same_from_here(dv, twin, case, k):
    """pixel_state and running_intensities equal the twin's, and so do the next accepted push and the finish."""
    a, b = dv.pixel_state(), twin.pixel_state()
    assert np.array_equal(a[0], b[0]) and np.array_equal(bits(a[1]), bits(b[1]))
    assert np.array_equal(dv.running_intensities(), twin.running_intensities())
    want = oracle(case["name"])[0][k]
    for d in (dv, twin):
        got = push(d, case["packets"][k])
        assert got.tobytes() == want["events"].tobytes()
        check_state(d, want)
    assert dv.finish().tobytes() == twin.finish().tobytes()


@pytest.mark.parametrize("what", ["before", "after", "nan", "minus_one", "capacity"])
def test_refused_push_changes_nothing(what):
    case = BY_NAME["seeded_mode1"]
    k = 2
    dv, twin = _twin(case, k), _twin(case, k)
    pk = dict(case["packets"][k])
    nb = len(pk["before"])
    with pytest.raises(A.AdderHipError) as ei:
        if what == "before":
            pk["before"] = pk["before"].copy()
            pk["before"]["x"][[7, 300]] = case["W"]
            push(dv, pk)
        elif what == "after":
            pk["after"] = pk["after"].copy()
            pk["after"]["y"][[5, 9]] = case["H"]
            push(dv, pk)
        elif what in ("nan", "minus_one"):
            pk["frame"] = pk["frame"].copy()
            pk["frame"][3, 4] = np.nan if what == "nan" else -1.0
            push(dv, pk)
        else:
            push(dv, pk, out_cap=dv.push_capacity(nb) - 1)
    e = ei.value
    if what == "before":
        assert e.code == D.E_BAD_EVENT and e.index == 7 == dv.bad_index
    elif what == "after":
        assert e.code == D.E_BAD_EVENT and e.index == nb + 5
    elif what == "capacity":
        assert e.code == A.E_OUT_CAPACITY and e.needed == dv.push_capacity(nb)
        want = oracle(case["name"])[0][k]
        got = push(dv, case["packets"][k], out_cap=e.needed)  # the repeat at *n_out succeeds
        assert got.tobytes() == want["events"].tobytes()
        push(twin, case["packets"][k])
        k += 1
    else:
        assert e.code == A.E_BAD_PARAMS
    _same_from_here(dv, twin, case, k)
    dv.close()
    twin.close()


def test_push_after_finish_is_an_order_error_and_reset_starts_over():
    case = BY_NAME["seeded_mode2"]
    res, fin, _ = oracle(case["name"])
    dv = make(case)
    first = [push(dv, pk) for pk in case["packets"][:3]]
    end = dv.finish()
    state, running = dv.pixel_state(), dv.running_intensities()
    for call in (lambda: push(dv, case["packets"][3]), dv.finish):
        with pytest.raises(A.AdderHipError) as ei:
            call()
        assert ei.value.code == D.E_ORDER
    after = dv.pixel_state()
    assert np.array_equal(state[0], after[0]) and np.array_equal(bits(state[1]), bits(after[1]))
    assert np.array_equal(running, dv.running_intensities())
    dv.reset()
    ts, ln = dv.pixel_state()
    assert not ts.any() and not bits(ln).any()
    again = [push(dv, pk) for pk in case["packets"][:3]]
    assert [a.tobytes() for a in again] == [f.tobytes() for f in first] == [r["events"].tobytes() for r in res[:3]]
    assert dv.finish().tobytes() == end.tobytes()
    dv.close()


def test_create_refuses_a_height_that_is_no_multiple_of_four():
    with pytest.raises(A.AdderHipError) as ei:
        D.HipDavis(38, 30, D.RAW_DAVIS, DC.TPS, DC.REF, DC.DTM)
    assert ei.value.code == A.E_BAD_PARAMS and "multiple of 4" in str(ei.value)


def _mirror_device(packets, width, height, mode, *, tps, ref_time, delta_t_max, crf):
    """adder_host_davis_device: the mirror's Davis with chain_on_device(true); host_py.davis's layout of the arguments."""
    import host_py as Hst
    P = len(packets)
    frames = np.ascontiguousarray(np.stack([p["frame"] for p in packets]).astype(np.float64))
    meta = np.zeros(P, Hst.DAVIS_META_DTYPE)
    dvs = []
    for k, p in enumerate(packets):
        meta[k] = (p["c"], p["start"], p["end"], len(p["before"]), len(p["after"]))
        dvs += [np.ascontiguousarray(p["before"], Hst.DAVIS_DVS_DTYPE), np.ascontiguousarray(p["after"], Hst.DAVIS_DVS_DTYPE)]
    dvs = np.concatenate(dvs)
    cap = max(4096, (len(dvs) * 4 + (3 * P + 2) * width * height) * 6)
    out = np.zeros(cap, A.EVENT_DTYPE)
    ret = C.c_ulonglong(0)
    fn = Hst.lib().adder_host_davis_device
    fn.restype = C.c_longlong
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint16, C.c_uint16, C.c_int, C.c_uint32, C.c_uint32,
                   C.c_uint32, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_ulonglong)]
    n = fn(frames.ctypes.data, meta.ctypes.data, dvs.ctypes.data, P, width, height, mode, tps, ref_time, delta_t_max, 1,
           -1 if crf is None else crf, out.ctypes.data, cap, C.byref(ret))
    if n < 0:
        raise RuntimeError(Hst.err())
    assert n <= cap
    return out[:n].copy(), ret.value


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_mirror_with_the_chain_on_the_device_returns_the_mirror_off_events(mode):
    import host_py as Hst
    case = DC.SEEDED[mode]
    kw = dict(tps=case["tps"], ref_time=case["ref_time"], delta_t_max=case["dtm"], crf=case["crf"])
    off, off_returned = Hst.davis(case["packets"], case["W"], case["H"], mode, **kw)
    on, on_returned = _mirror_device(case["packets"], case["W"], case["H"], mode, **kw)
    assert len(on) == len(off) > 2 * case["W"] * case["H"] and on.tobytes() == off.tobytes()
    assert on_returned == off_returned > 0


def test_file_tool_output_reads_back_as_the_events(tmp_path):
    import adder_stream_np as S
    case = BY_NAME["seeded_mode1"]
    want = oracle(case["name"])[2]
    out = str(tmp_path / "davis.adder")
    info = A.davis_to_adder_file(case["packets"], out, case["W"], case["H"], case["mode"], tps=case["tps"],
                                 ref_time=case["ref_time"], delta_t_max=case["dtm"], crf=case["crf"])
    assert info["events"] == len(want) and info["packets"] == len(case["packets"])
    meta, ev, closed = S.read_adder(open(out, "rb").read())
    assert closed and (meta["width"], meta["height"], meta["channels"]) == (case["W"], case["H"], 1)
    assert meta["source_camera"] == D.SOURCE_CAMERA_DAVIS_U8 and meta["tps"] == case["tps"]
    assert np.array_equal(ev, want)
    got = A.davis_to_adder(case["packets"], case["W"], case["H"], case["mode"], tps=case["tps"], ref_time=case["ref_time"],
                           delta_t_max=case["dtm"], crf=case["crf"])
    assert got.tobytes() == want.tobytes()
