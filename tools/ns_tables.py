#!/usr/bin/env python3
"""Generates csrc/igdsp_ns_tab.h, the noise suppressor's window and twiddle tables (include/igdsp.h, "Noise suppression").

    python tools/ns_tables.py            # print the SHA-256 of the tables and compare the committed header
    python tools/ns_tables.py --write    # rewrite the header

Both tables are made in float64 and rounded once to the nearest integer: the sine window w[i] = round(32768 sin(pi (i + 0.5) / 160)),
i = 0 .. 159, as int16 (the largest entry is 32767: w[i]^2 + w[i + 80]^2 = 2^30 up to that rounding), and the twiddle factors
t[k] = (round(2^30 cos(2 pi k / 256)), round(2^30 sin(2 pi k / 256))), k = 0 .. 127, as int32 pairs (Q30; the 128-point passes read the
even k).  The committed constants are the definition: tests/test_ns_cpu.py pins their SHA-256 and compares them with float64 numpy."""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "igate4xsoftphonedsp_amd", "csrc", "igdsp_ns_tab.h")
WIN, HALF = 160, 128


def window():
    return np.rint(32768.0 * np.sin(np.pi * (np.arange(WIN) + 0.5) / WIN)).astype(np.int16)


def twiddle():
    a = 2.0 * np.pi * np.arange(HALF) / (2 * HALF)
    return np.rint(np.stack([np.cos(a), np.sin(a)], axis=1) * float(1 << 30)).astype(np.int32)      # [128][2]


def digest():
    d = hashlib.sha256()
    d.update(window().astype("<i2").tobytes())
    d.update(twiddle().astype("<i4").tobytes())
    return d.hexdigest()


def values(name, v):
    rows = [", ".join(str(int(x)) for x in v[i:i + 8]) for i in range(0, len(v), 8)]
    return f"#define {name} \\\n    " + ", \\\n    ".join(rows) + "\n"


def header():
    out = ["// igdsp_ns_tab.h — the noise suppressor's tables (include/igdsp.h, \"Noise suppression\"): IGDSP_NS_WIN_VALUES is the sine window\n"
           "// w[i] = round(32768 sin(pi (i + 0.5) / 160)), i = 0 .. 159 (int16); IGDSP_NS_TW_VALUES is t[k] = (round(2^30 cos(2 pi k / 256)),\n"
           "// round(2^30 sin(2 pi k / 256))), k = 0 .. 127, as re, im pairs (int32, Q30).  Made in float64 and rounded once: nothing is computed at\n"
           "// run time, the host and the device read the same bits.  Made by tools/ns_tables.py; THESE CONSTANTS ARE THE DEFINITION,\n"
           "// tests/test_ns_cpu.py pins their SHA-256\n"
           f"// ({digest()}).\n"
           "#pragma once\n"]
    out.append(values("IGDSP_NS_WIN_VALUES", window()))
    out.append(values("IGDSP_NS_TW_VALUES", twiddle().reshape(-1)))
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
