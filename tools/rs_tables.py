#!/usr/bin/env python3
"""Generates csrc/igdsp_rs_tab.h, the rate converter's Q14 tap tables (include/igdsp.h, "Rate converter").

    python tools/rs_tables.py            # print the SHA-256 of the tables and compare the committed header
    python tools/rs_tables.py --write    # rewrite the header

The float64 formula below is how the constants are made; the committed constants are the definition (tests/test_rs_cpu.py pins their
SHA-256 and compares them with tests/rs_model.py, which restates the formula on its own)."""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "igate4xsoftphonedsp_amd", "csrc", "igdsp_rs_tab.h")
FACTORS, TAPS, CUTOFF, BETA = (2, 3, 4, 6), 24, 0.95, 6.0


def prototype(R):
    N = TAPS * R
    c = np.arange(N) - (N - 1) / 2
    return np.sinc(CUTOFF * c / R) * np.kaiser(N, BETA)


def fix(v):
    q = np.floor(16384.0 * v / v.sum() + 0.5).astype(np.int64)
    q[int(np.argmax(np.abs(q)))] += 16384 - int(q.sum())       # argmax: the lowest index on a tie
    return q


def tables(R):
    h = prototype(R)
    return np.stack([fix(h[p::R]) for p in range(R)]), fix(h)


def digest():
    d = hashlib.sha256()
    for R in FACTORS:
        up, down = tables(R)
        d.update(up.astype("<i2").tobytes())
        d.update(down.astype("<i2").tobytes())
    return d.hexdigest()


def values(name, v):
    rows = [", ".join(str(int(x)) for x in v[i:i + 24]) for i in range(0, len(v), 24)]
    return f"#define {name} \\\n    " + ", \\\n    ".join(rows) + "\n"


def header():
    out = ["// igdsp_rs_tab.h — the rate converter's tap tables (include/igdsp.h, \"Rate converter\"): Q14, 24 taps per phase, factors 2, 3, 4, 6.\n"
           "// IGDSP_RS_UPr_VALUES is U_r[p][k] in [p][k] order (r x 24 values), IGDSP_RS_DOWNr_VALUES is D_r[j] (24 r values).  Every phase of\n"
           "// an up table and every down table sums to 16384.  Lists of constants: nothing is computed at run time, the host and the device\n"
           "// read the same bits.  Made by tools/rs_tables.py; THESE CONSTANTS ARE THE DEFINITION, tests/test_rs_cpu.py pins their SHA-256\n"
           f"// ({digest()}).\n"
           "#pragma once\n"]
    for R in FACTORS:
        up, down = tables(R)
        out.append(values(f"IGDSP_RS_UP{R}_VALUES", up.reshape(-1)))
        out.append(values(f"IGDSP_RS_DOWN{R}_VALUES", down))
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
