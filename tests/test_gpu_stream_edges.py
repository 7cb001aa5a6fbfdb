"""The stream tools (include/adder_stream.h) at their edges on the MI355X: every case of tests/stream_edge_cases.py
through every entry point that can carry it -- AdderEvents and wire records, host and device forms, out of place and in
place -- byte for byte and bit for bit against the restatement, batch after batch on one handle, so that each batch
behind a bad or EOF record also checks the state the call left.  Device outputs start as 0xA5: what a call must not
write is still 0xA5 (or still the input, in place) afterwards.  Then the two file tools with batches that end on, before
and behind the EOF record.

One handle per (metadata, operation), reset between runs; no transcoder context, no captured graph; the largest input
is 6 000 events.  Bad events are defined error returns: their keys are the sentinel, so they address nothing."""
import ctypes as C
import struct

import numpy as np
import pytest

import adder_stream_np as S
import stream_edge_cases as E
import stream_tools_oracle as R
from test_stream_tools_cpu import lib_meta

pytestmark = pytest.mark.gpu

CASES = E.all_cases()
FILL = 0xA5
NO_BAD = (1 << 64) - 1
_HANDLES = {}


@pytest.fixture(scope="module", autouse=True)
def _handles_closed_at_the_end():
    yield
    for h in _HANDLES.values():
        h.close()
    _HANDLES.clear()


def handle(meta, op):
    """the one handle of this metadata and operation, its state forgotten"""
    from adder_amd import stream_tools as T
    key = (tuple(sorted(lib_meta(meta).items())), "info" if op == "info" else E.out_mode(meta, op))
    if key not in _HANDLES:
        _HANDLES[key] = T.HipStreamInfo(**lib_meta(meta)) if op == "info" else \
            T.HipStreamMigrator(out_time_mode=E.out_mode(meta, op), **lib_meta(meta))
    h = _HANDLES[key]
    h.reset()
    return h


def bits(x):
    return struct.pack("<d", x)


def batch_bytes(c, source, k):
    a, b = c["cuts"][k], c["cuts"][k + 1]
    if source == "events":
        return c["events"][a:b].tobytes(), 12
    rb = c["record_bytes"]
    return c["body"][rb * a:rb * b], rb


def call(h, op, source, form, data, n):
    """one batch through the C-ABI.  -> (rc, bad, consumed or None, output bytes or None, the input after the call)"""
    import torch
    L, info = h.L, op == "info"
    bad, consumed = C.c_uint64(7), C.c_uint64(7)
    src = np.frombuffer(data, np.uint8).copy()
    if form == "host":
        dst = np.full(len(src), FILL, np.uint8)
        if source == "events":
            rc = L.adder_stream_info_host(h.h, src.ctypes.data, n, C.byref(bad)) if info else \
                L.adder_stream_migrate_host(h.h, src.ctypes.data, n, dst.ctypes.data, C.byref(bad))
        else:
            rc = L.adder_stream_info_wire_host(h.h, src.ctypes.data, n, C.byref(bad), C.byref(consumed)) if info else \
                L.adder_stream_migrate_wire_host(h.h, src.ctypes.data, n, dst.ctypes.data, C.byref(bad),
                                                 C.byref(consumed))
        out, after = dst.tobytes(), src.tobytes()
    else:
        d_in = torch.from_numpy(src).cuda()
        d_out = d_in if form == "device_in_place" else torch.full_like(d_in, FILL)
        if source == "events":
            rc = L.adder_stream_info_device(h.h, d_in.data_ptr(), n, C.byref(bad), None) if info else \
                L.adder_stream_migrate_device(h.h, d_in.data_ptr(), n, d_out.data_ptr(), C.byref(bad), None)
        else:
            rc = L.adder_stream_info_wire_device(h.h, d_in.data_ptr(), n, C.byref(bad), C.byref(consumed), None) \
                if info else L.adder_stream_migrate_wire_device(h.h, d_in.data_ptr(), n, d_out.data_ptr(),
                                                                C.byref(bad), C.byref(consumed), None)
        out, after = d_out.cpu().numpy().tobytes(), d_in.cpu().numpy().tobytes()
    return rc, bad.value, (None if source == "events" else consumed.value), (None if info else out), after


def forms_of(op):
    return ("host", "device") if op == "info" else ("host", "device", "device_in_place")


def run_case(c, verbose=False):
    for source in (("events", "wire") if c["events"] is not None else ("wire",)):
        for op in c["ops"]:
            want = E.expected(c, op, source)
            for form in forms_of(op):
                h = handle(c["meta"], op)
                for k, r in enumerate(want):
                    data, rb = batch_bytes(c, source, k)
                    where = (c["name"], source, op, form, k)
                    assert r["n"] > 0
                    rc, bad, consumed, out, after = call(h, op, source, form, data, r["n"])
                    assert rc == r["rc"], where
                    assert bad == (NO_BAD if r["bad"] is None else r["bad"]), where
                    if source == "wire":
                        assert consumed == r["consumed"], where
                    if op == "info":
                        lo, hi, cnt = h.range()
                        assert (bits(lo), bits(hi), cnt) == (bits(r["range"][0]), bits(r["range"][1]), r["range"][2]), where
                        assert after == data, where
                        continue
                    cut = r["done"] * rb
                    assert out[:cut] == r["out"], where  # whole records: every byte but t's four is the input's
                    # from the first bad / EOF record on nothing is written
                    rest = data[cut:] if form == "device_in_place" else bytes([FILL]) * (len(data) - cut)
                    assert out[cut:] == rest, where
                    if form != "device_in_place":
                        assert after == data, where


@pytest.mark.parametrize("name", E.names("tags"))
def test_wire11_tags(name):
    run_case(CASES[name])


def test_tag0_records_out_of_place_are_whole():
    """A None record (tag 0) keeps all 11 bytes but the four of t -- byte 10, behind t, too -- in the device form with
    a separate output buffer, forward, inverse and passed through."""
    import torch
    for name, ops in (("tags_mixed/dt", ("forward", "pass_same", "pass_mixed")), ("tags_mixed/abs", ("inverse",))):
        c = CASES[name]
        body = np.frombuffer(c["body"], np.uint8).reshape(-1, 11)
        zero = body[:, 4] == 0
        assert zero.sum() > 100 and (body[zero, 10] != 0).all()
        for op in ops:
            h = handle(c["meta"], op)
            d_in = torch.from_numpy(body.reshape(-1).copy()).cuda()
            d_out = torch.full_like(d_in, FILL)
            bad, consumed = C.c_uint64(0), C.c_uint64(0)
            rc = h.L.adder_stream_migrate_wire_device(h.h, d_in.data_ptr(), len(body), d_out.data_ptr(), C.byref(bad),
                                                      C.byref(consumed), None)
            assert (rc, bad.value, consumed.value) == (0, NO_BAD, len(body))
            got = d_out.cpu().numpy().reshape(-1, 11)
            keep = [0, 1, 2, 3, 4, 5, 10]  # x, y, tag, d and the byte behind t
            assert np.array_equal(got[zero][:, keep], body[zero][:, keep]), op
            assert np.array_equal(got[~zero][:, :7], body[~zero][:, :7]), op
            if op.startswith("pass"):
                assert np.array_equal(got, body), op


@pytest.mark.parametrize("name", E.names("units"))
def test_sentinel_keys_at_unit_counts(name):
    run_case(CASES[name])


@pytest.mark.parametrize("name", E.names("grid"))
def test_grid_edges(name):
    run_case(CASES[name])


@pytest.mark.parametrize("name", E.names("errors"))
def test_error_interplay(name):
    run_case(CASES[name])


@pytest.mark.parametrize("stem", sorted({n.split("/")[0] for n in E.names("time")}))
def test_time_edges(stem):
    for how in ("whole", "cut"):
        run_case(CASES[f"{stem}/{how}"])


@pytest.mark.parametrize("word", ["dt", "abs"])
def test_fold_arms(word):
    run_case(CASES[f"fold_6000/{word}"])
    for k in range(12):
        run_case(CASES[f"fold_12_cut{k}/{word}"])


# ---- the file tools at batch edges --------------------------------------------------------------------------------------

FILE_EVENTS = 300
FILE_BATCHES = (1, 299, 300, 301)  # the EOF record alone in a batch, second of two, first of the next, last of its own


def file_variant(ch, variant):
    """-> (file bytes, meta, the events in front of the end).  9-byte files end in the 11-byte EOF record, whose last two
    bytes a batch of 301 records leaves unread."""
    meta = E.meta_of(5, 4, ch)
    rng = np.random.default_rng([17, ch])
    ev = E.random_events(rng, meta, FILE_EVENTS)
    ev["pad"] = 0
    whole = S.write_adder(meta, ev, close=False)
    hdr = len(S.build_header(meta))
    rb = 9 if ch == 1 else 11
    if variant == "closed":
        return whole + S.EOF, meta, ev
    if variant == "no_eof":
        return whole, meta, ev
    if variant == "truncated":
        return whole + whole[hdr:hdr + rb - 4], meta, ev
    assert variant == "eof_first"
    return whole[:hdr] + S.EOF + whole[hdr:], meta, ev[:0]


@pytest.mark.parametrize("variant", ["closed", "no_eof", "truncated", "eof_first"])
@pytest.mark.parametrize("ch", [1, 3])
def test_file_tools_at_batch_edges(tmp_path, ch, variant):
    import adder_amd as A
    buf, meta, ev = file_variant(ch, variant)
    hdr = len(S.build_header(meta))
    src = tmp_path / "in.adder"
    src.write_bytes(buf)
    out, bad = R.Migration(meta, R.ABSOLUTE_T).run(ev)
    assert bad is None
    want = R.migrated_header(buf, R.ABSOLUTE_T) + S.encode_records(E.with_times(ev, out), ch) + R.EOF
    info = R.Info(meta)
    assert info.run(ev) is None
    text = R.report(meta, hdr, len(buf), len(ev), True, info.min, info.max)
    for batch in FILE_BATCHES:
        dst = tmp_path / f"out_{batch}.adder"
        assert A.migrate_file(str(src), str(dst), "absolute", batch_records=batch) == dict(events=len(ev)), batch
        assert dst.read_bytes() == want, batch
        assert A.adder_info_file(str(src), True, batch_records=batch) == text, batch
    dst = tmp_path / "mixed.adder"
    assert A.migrate_file(str(src), str(dst), "mixed", batch_records=299) == dict(events=len(ev))
    assert dst.read_bytes() == R.migrated_header(buf, R.MIXED) + S.encode_records(ev, ch) + R.EOF
