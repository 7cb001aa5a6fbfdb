"""The three raw-header parsers of the C-ABI (adder_dvs_parse_header, adder_stream_parse_header,
adder_player_parse_header) against the independent numpy reader tests/adder_stream_np.py.  Host code only: no GPU.

They share one parse (csrc/adder_api_util.hpp: raw_header_parse) and differ in what each refuses on top of it; the
difference -- a time mode above 2 -- is asserted here so that it stays a decision."""
import ctypes as C

import pytest

import adder_stream_np as S

TOOLS = ("dvs", "stream", "player")
# which of the numpy reader's fields each tool's params struct carries, by the struct's field name
FIELDS = {
    "dvs": dict(width="width", height="height", channels="channels", ref_interval="ref_interval",
                source_camera="source_camera", time_mode="time_mode"),
    "stream": dict(width="width", height="height", channels="channels", ref_interval="ref_interval",
                   source_camera="source_camera", time_mode="time_mode", out_time_mode="time_mode", tps="tps",
                   delta_t_max="delta_t_max", codec_version="version"),
    "player": dict(width="width", height="height", channels="channels", ref_interval="ref_interval",
                   source_camera="source_camera", time_mode="time_mode", tps="tps"),
}


def tool(name):
    from adder_amd import dvs, player, stream_tools
    mod, params, fn = {"dvs": (dvs, dvs.AdderDvsParams, "adder_dvs_parse_header"),
                       "stream": (stream_tools, stream_tools.AdderStreamParams, "adder_stream_parse_header"),
                       "player": (player, player.AdderPlayerParams, "adder_player_parse_header")}[name]
    return getattr(mod.load(), fn), params


def parse(name, buf, length=None):
    """-> (rc, params, header bytes, event bytes) of the tool's parser over buf[:length]"""
    fn, params = tool(name)
    p, hb, eb = params(), C.c_uint32(0), C.c_uint32(0)
    b = bytes(buf) + b"\0" * 8  # the bytes behind `length` exist: a parser that read past it would not fault here
    rc = fn(b, len(buf) if length is None else length, C.byref(p), C.byref(hb), C.byref(eb))
    return rc, p, hb.value, eb.value


def header(version, channels, time_mode=1):
    # every byte of every multi-byte field distinct: a swapped or shifted read shows
    return S.build_header(dict(version=version, width=0x0123, height=0x0245, tps=0x01020304, ref_interval=0x05060708,
                               delta_t_max=0x090A0B0C, channels=channels, source_camera=0x0D0E0F10,
                               time_mode=time_mode, adu_interval=0x11121314))


@pytest.mark.parametrize("channels", (1, 3))
@pytest.mark.parametrize("version", (0, 1, 2, 3))
@pytest.mark.parametrize("name", TOOLS)
def test_parse_header_accepts_what_the_numpy_reader_reads_and_refuses_the_rest(name, version, channels):
    buf = header(version, channels)
    want = S.parse_header(buf)
    assert want["header_size"] == len(buf) == 25 + 4 * version
    for extra in (b"", b"\xaa" * 7):  # the exact length, and with a body behind it
        rc, p, hb, eb = parse(name, buf + extra)
        assert rc == 0
        assert hb == want["header_size"] and eb == want["event_size"] == (9 if channels == 1 else 11)
        for field, key in FIELDS[name].items():
            assert getattr(p, field) == want[key], (field, key)
        assert p.device_id == 0

    def refused(b, length=None):
        return parse(name, b, length)[0] == -1  # ADDER_E_BAD_PARAMS

    assert refused(buf, 24) and refused(buf, 25 + 4 * version - 1) and refused(buf, 0)
    assert refused(b"addec" + buf[5:]) and refused(b"Adder" + buf[5:])
    assert refused(buf[:6] + b"l" + buf[7:])
    assert refused(buf[:5] + b"\x04" + buf[6:] + b"\0" * 4)
    assert refused(header(version, 3)[:23] + b"\x09" + header(version, 3)[24:])  # 9-byte events, 3 channels
    assert refused(header(version, 1)[:23] + b"\x0b" + header(version, 1)[24:])  # 11-byte events, 1 channel
    assert refused(header(version, 0))


@pytest.mark.parametrize("name", TOOLS)
def test_time_mode_above_2_is_refused_by_the_stream_tool_alone(name):
    """The stream tool rewrites the time mode and refuses one it does not know.  The DVS converter and the player
    keep the field's low byte and leave the judgement to their create call."""
    for version in (2, 3):
        for mode in (3, 0x0103):
            rc, p, _, _ = parse(name, header(version, 1, time_mode=mode))
            if name == "stream":
                assert rc == -1
            else:
                assert rc == 0 and p.time_mode == 3
        rc, p, _, _ = parse(name, header(version, 1, time_mode=2))
        assert rc == 0 and p.time_mode == 2
    # below version 2 the header has no such field: nothing to refuse
    rc, p, _, _ = parse(name, header(1, 1, time_mode=3))
    assert rc == 0 and p.time_mode == 0
