"""csrc/kernels/aiko_api.h is the one declaration of every extern "C" aiko_* launcher.

The compiler checks a declaration against its definition only where both are seen together, and
it says nothing about a definition that has no declaration at all.  These text checks close the
gap: every launcher a kernel file defines is declared in the header, every such file includes the
header, and nobody else declares a launcher by hand.
"""
import re
from pathlib import Path

CSRC = Path(__file__).resolve().parent.parent / "aiko_services_amd" / "csrc"
API = CSRC / "kernels" / "aiko_api.h"

# a function head at the start of a line: return type, aiko_ name, parameters, then ';' or '{'
HEAD = re.compile(r"^(?:extern \"C\" )?(?:const )?[A-Za-z_][\w:]*[\s*&]+(aiko_\w+)\s*\(([^()]*)\)\s*([;{])", re.M)


def _strip_comments(text):
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return re.sub(r"//[^\n]*", "", text)


def _extern_c_text(text):
    """The parts of ``text`` with C linkage: extern "C" { ... } blocks and extern "C" one-liners."""
    out = []
    for m in re.finditer(r'extern "C"\s*\{', text):
        depth, i = 1, m.end()
        while depth and i < len(text):
            depth += {"{": 1, "}": -1}.get(text[i], 0)
            i += 1
        out.append(text[m.end():i])
    out += [m.group(0) for m in re.finditer(r'^extern "C" [^{;]*[{;]', text, re.M)]
    return "\n".join(out)


def _heads(path, c_linkage_only):
    text = _strip_comments(path.read_text())
    if c_linkage_only:
        text = _extern_c_text(text)
    return [(m.group(1), m.group(3)) for m in HEAD.finditer(text)]


def _defined(path):
    return {name for name, end in _heads(path, True) if end == "{"}


def test_every_launcher_is_declared_in_the_header():
    declared = {name for name, end in _heads(API, True) if end == ";"}
    assert len(declared) >= 60
    missing = {}
    for hip in sorted((CSRC / "kernels").glob("*.hip")):
        gap = _defined(hip) - declared
        if gap:
            missing[hip.name] = sorted(gap)
    assert not missing, f"extern \"C\" launchers without a declaration in aiko_api.h: {missing}"
    defined = set().union(*(_defined(h) for h in (CSRC / "kernels").glob("*.hip")))
    assert declared == defined, f"declared but defined nowhere: {sorted(declared - defined)}"


def test_every_defining_file_includes_the_header():
    files = [h for h in sorted((CSRC / "kernels").glob("*.hip")) if _defined(h)]
    assert len(files) >= 30
    without = [h.name for h in files if not re.search(r'^#include "aiko_api\.h"', h.read_text(), re.M)]
    assert not without, f"kernel files that define launchers without including aiko_api.h: {without}"


def test_nobody_else_declares_a_launcher():
    stray = {}
    for path in sorted(CSRC.rglob("*")):
        if path.suffix not in (".h", ".hpp", ".hip", ".cpp", ".c", ".cc") or path == API:
            continue
        found = sorted(name for name, end in _heads(path, False) if end == ";")
        if found:
            stray[str(path.relative_to(CSRC))] = found
    assert not stray, f"aiko_* prototypes outside aiko_api.h: {stray}"
