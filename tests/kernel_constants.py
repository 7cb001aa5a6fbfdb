"""The launch-geometry constants of the quality, framer, stream hand-off, display and band records kernels, read from their sources, so the edge tests take
their shapes from the values the kernels are built with: a retune moves the tests with it.  A name that is missing, or
an expression this cannot evaluate, raises."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "adder-codec-rs_amd", "csrc")

QUALITY_NAMES = ("kQualBlock", "kSsimTileW", "kSsimTileH", "kSseBytesPerBlock", "kSseMaxBlocks")
FRAMER_NAMES = ("kFramerPopMaxBlocks", "kFramerPopUnitsPerBlock", "kFramerPopWideUnitsPerBlock",
                "kFramerMinmaxMaxBlocks", "kFramerMinmaxUnitsPerBlock")
DISPLAY_NAMES = ("kDisplayRows", "kDisplayTileBytes")
HANDOFF_NAMES = ("kBlockThreads", "kWireEvents", "kScatterGroupsPerCu", "kMergeTileFrames", "kMaxGridRows")
RECORDS_NAMES = ("kWaveUnits", "kExpandSegs", "kMaxBands", "kMaxChunk")

_DECL = re.compile(r"^\s*constexpr\s+uint32_t\s+(\w+)\s*=\s*([^;]+);", re.M)
_ARITH = re.compile(r"[0-9+\-*/() ]+")
_MACRO = re.compile(r"^\s*#\s*define\s+(\w+)\s+(\d+)[uU]?\s*(?://.*)?$", re.M)
_MEMBER = re.compile(r"^\s*static\s+constexpr\s+uint32_t\s+(\w+)\s*=\s*(\d+)[uU]?\s*;", re.M)


def parse_u32_constants(text, names, macros=False):
    """{name: value} of the `constexpr uint32_t name = expr;` lines of a header; expr may be integer arithmetic over
    literals (with a u suffix) and names declared above it -- with `macros`, also over the header's `#define NAME
    <integer>` lines (the first definition of a name: the default behind its #ifndef)."""
    seen = {}
    if macros:
        for name, value in _MACRO.findall(text):
            seen.setdefault(name, int(value))
    for name, expr in _DECL.findall(text):
        e = re.sub(r"\b(\d+)[uU]\b", r"\1", expr)
        e = re.sub(r"\b[A-Za-z_]\w*\b", lambda m: str(seen[m.group(0)]) if m.group(0) in seen else m.group(0), e)
        if _ARITH.fullmatch(e):
            seen[name] = int(eval(e.replace("/", "//"), {"__builtins__": {}}))
    missing = [n for n in names if n not in seen]
    if missing:
        raise KeyError(f"constants not found (or not plain integer arithmetic): {missing}")
    return {n: seen[n] for n in names}


def _read(header, names):
    with open(os.path.join(CSRC, header)) as f:
        return parse_u32_constants(f.read(), names)


def quality():
    return _read("adder_quality_kernels.h", QUALITY_NAMES)


def framer():
    return _read("adder_framer_kernels.h", FRAMER_NAMES)


def handoff():
    return _read("adder_kernels.h", HANDOFF_NAMES)


def records():
    """The band records path (adder_kernels.hip: the pack, layout and expand-bands kernels; adder_hip_records_api.cpp):
    segment size, segments per expansion wave, bands per launch, frames per chunk, and the root's description slots."""
    with open(os.path.join(CSRC, "adder_kernels.h")) as f:
        out = parse_u32_constants(f.read(), RECORDS_NAMES, macros=True)
    with open(os.path.join(CSRC, "adder_hip_ctx.hpp")) as f:
        members = dict(_MEMBER.findall(f.read()))
    if "kBandDescSlots" not in members:
        raise KeyError("constants not found: ['kBandDescSlots']")
    out["kBandDescSlots"] = int(members["kBandDescSlots"])
    return out


def display():
    return _read("adder_display.hip", DISPLAY_NAMES)
