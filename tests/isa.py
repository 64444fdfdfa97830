"""The generated code of a unit of arcquant_amd/csrc for the ISA audit tests: the one compile line (gfx950 assembly, product flags), a
per-process cache so that a unit is compiled at most once per test session, and what the audits share in reading the assembly."""
import os
import re
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "arcquant_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-S", "--cuda-device-only"]

_assembly = {}                      # unit (file name in csrc) -> text of its assembly


def assembly(*units):
    """Compiles those of `units` that this process has not compiled yet, side by side; returns the text of the first."""
    with tempfile.TemporaryDirectory() as out:
        procs = []
        for unit in dict.fromkeys(u for u in units if u not in _assembly):
            asm = os.path.join(out, unit + ".s")
            procs.append((unit, asm, subprocess.Popen([HIPCC, *FLAGS, "-I", CSRC, os.path.join(CSRC, unit), "-o", asm], stderr=subprocess.DEVNULL)))
        for unit, asm, proc in procs:
            assert proc.wait() == 0, unit
            with open(asm) as f:
                _assembly[unit] = f.read()
    return _assembly[units[0]]


def kernel(unit, symbol):
    """(code, metadata) of kernel `symbol` of `unit`: its instructions and labels, and its .amdhsa_kernel block."""
    text = assembly(unit)
    a = text.index("\n" + symbol + ":")
    body = text[a:text.index(".end_amdhsa_kernel", a)]
    return body[:body.rindex(".amdhsa_kernel")], body[body.rindex(".amdhsa_kernel"):]


def _innermost_loop(code):
    """Instructions of the loop (label .. backward conditional branch to it) that holds the most v_mfma and no other loop."""
    lines = []
    for line in code.split("\n"):
        t = line.split(";")[0].strip()
        if t and (t.endswith(":") or not t.startswith(".")):
            lines.append(t)
    labels = {t[:-1]: i for i, t in enumerate(lines) if t.endswith(":")}
    loops = []
    for i, t in enumerate(lines):
        m = re.match(r"s_cbranch_\w+\s+(\S+)", t)
        if m and labels.get(m.group(1), i) < i:
            loops.append((labels[m.group(1)], i))
    assert loops, "no loop in the kernel"
    inner = [(a, b) for a, b in loops if not any((c, d) != (a, b) and a <= c and d <= b for c, d in loops)]
    a, b = max(inner, key=lambda ab: sum(t.startswith("v_mfma") for t in lines[ab[0]:ab[1]]))
    return [t for t in lines[a:b] if not t.endswith(":")]
