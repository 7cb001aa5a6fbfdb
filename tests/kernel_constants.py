"""The launch-geometry constants of the quality, framer, stream hand-off and display kernels, read from their sources, so the edge tests take
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

_DECL = re.compile(r"^\s*constexpr\s+uint32_t\s+(\w+)\s*=\s*([^;]+);", re.M)
_ARITH = re.compile(r"[0-9+\-*/() ]+")


def parse_u32_constants(text, names):
    """{name: value} of the `constexpr uint32_t name = expr;` lines of a header; expr may be integer arithmetic over
    literals (with a u suffix) and names declared above it."""
    seen = {}
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


def display():
    return _read("adder_display.hip", DISPLAY_NAMES)
