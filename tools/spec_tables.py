#!/usr/bin/env python3
"""Generates csrc/igdsp_spec_tab.h, the spectrum stage's window and twiddle tables (include/igdsp.h, "Spectrum").

    python tools/spec_tables.py            # print the SHA-256 of the tables and compare the committed header
    python tools/spec_tables.py --write    # rewrite the header

Both tables are made in float64 and rounded once to float32: the periodic Hann window w[i] = 0.5 - 0.5 cos(2 pi i / 1024), i = 0 .. 1023,
and the twiddle factors t[k] = (cos(2 pi k / 1024), -sin(2 pi k / 1024)), k = 0 .. 1023 (values below 1e-15 in magnitude, the float64
residue at the quadrant points, are written as 0).  The committed constants are the definition: tests/test_spec_cpu.py pins their
SHA-256 and compares the window with the one tests/spec_model.py builds on its own."""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "igate4xsoftphonedsp_amd", "csrc", "igdsp_spec_tab.h")
N = 1024


def window():
    return (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(N) / N)).astype(np.float32)


def twiddle():
    a = 2.0 * np.pi * np.arange(N) / N
    t = np.stack([np.cos(a), -np.sin(a)], axis=1)
    t[np.abs(t) < 1e-15] = 0.0
    return t.astype(np.float32)                      # [1024][2]


def digest():
    d = hashlib.sha256()
    d.update(window().astype("<f4").tobytes())
    d.update(twiddle().astype("<f4").tobytes())
    return d.hexdigest()


def lit(x):
    """a float32 as a C hex float literal: exact"""
    x = float(x)
    if x == 0.0:
        return "0.0f"
    m, e = x.hex().split("p")
    m = m.rstrip("0")
    return (m[:-1] if m.endswith(".") else m) + "p" + e + "f"


def values(name, v):
    rows = [", ".join(lit(x) for x in v[i:i + 8]) for i in range(0, len(v), 8)]
    return f"#define {name} \\\n    " + ", \\\n    ".join(rows) + "\n"


def header():
    out = ["// igdsp_spec_tab.h — the spectrum stage's tables (include/igdsp.h, \"Spectrum\"): IGDSP_SPEC_WIN_VALUES is the periodic Hann window\n"
           "// w[i] = 0.5 - 0.5 cos(2 pi i / 1024), i = 0 .. 1023; IGDSP_SPEC_TW_VALUES is t[k] = (cos(2 pi k / 1024), -sin(2 pi k / 1024)),\n"
           "// k = 0 .. 1023, as re, im pairs.  Made in float64 and rounded once to float, written as hex float literals: nothing is computed at run\n"
           "// time (no sinf, no cosf), the host and the device read the same bits.  Made by tools/spec_tables.py; THESE CONSTANTS ARE THE\n"
           "// DEFINITION, tests/test_spec_cpu.py pins their SHA-256\n"
           f"// ({digest()}).\n"
           "#pragma once\n"]
    out.append(values("IGDSP_SPEC_WIN_VALUES", window()))
    out.append(values("IGDSP_SPEC_TW_VALUES", twiddle().reshape(-1)))
    return "".join(out)


if __name__ == "__main__":
    text = header()
    print("sha256", digest())
    if "--write" in sys.argv:
        with open(HEADER, "w") as f:
            f.write(text)
        print("wrote", HEADER)
    else:
        same = os.path.exists(HEADER) and open(HEADER).read() == text
        print("header", "matches" if same else "DIFFERS")
        sys.exit(0 if same else 1)
