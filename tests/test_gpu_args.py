"""-m gpu: the rows of tests/args_cases.py that launch nothing (rejected, or nothing to do), replayed through the real library: the
code each entry returns.  Every pointer lies in one 64 KiB device buffer (a) and no kernel runs.  tests/test_args_cpu.py checks the same
table against csrc/igdsp_args.h without a device; this test ties the table to what the library does."""
import ctypes as C

import pytest

pytestmark = pytest.mark.gpu

from igate4xsoftphonedsp_amd import capi  # noqa: E402
from tests import args_cases as ac  # noqa: E402

CTYPE = {"p": C.c_void_p, "u": C.c_uint32, "q": C.c_uint64, "i": C.c_int, "win": C.POINTER(capi.Window), "cfg": C.c_void_p}
REPLAYED = [c for c in ac.CASES if c[3] == 0]


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(device=0, max_channels=64)
    yield c
    c.close()


@pytest.fixture(scope="module")
def a(ctx):
    p = ctx.dev_alloc(1 << 16)
    yield p
    ctx.dev_free(p)


@pytest.fixture(scope="module")
def entries(ctx):
    declared = {name for name, _, _ in capi.PROTOTYPES}
    fns = {}
    for entry, sig in ac.SIG.items():
        fn = getattr(ctx.L, ac.SYMBOL[entry])
        argtypes = [C.c_void_p] + [CTYPE[kind] for _, kind in sig] + [C.c_void_p]
        if ac.SYMBOL[entry] in declared:
            assert list(fn.argtypes) == argtypes, entry             # the table's parameter list is the binding's
        else:
            fn = capi.internal(ac.SYMBOL[entry])
            assert list(fn.argtypes) == argtypes, entry
        fns[entry] = fn
    return fns


def _value(kind, v, a):
    if kind == "p":
        v = str(v)
        return None if v == "0" else a + int(v[1:] or 0)
    return int(v)


def _call(fn, h, entry, kv, a):
    args, keep = ac.full(entry, kv), []
    out = []
    for key, kind in ac.SIG[entry]:
        if kind == "win":
            w = None
            if args["win"]:
                w = capi.Window(args["win.gate_mode"], args["win.probe_alarm"], *[_value("p", args[f"win.{f}"], a) for f in ac.WIN_FIELDS[2:]])
                keep.append(w)
            out.append(C.byref(w) if w is not None else None)
        elif kind == "cfg":
            c = None
            if args["cfg"]:
                c = (C.c_uint8 * 8)(*[args[f"cfg.{f}"] for f in ac.CFG_FIELDS], 0, 0, 0)
                keep.append(c)
            out.append(C.cast(c, C.c_void_p) if c is not None else None)
        else:
            out.append(_value(kind, args[key], a))
    return fn(h, *out, None)


def test_replay(ctx, a, entries):
    assert a % 4096 == 0 and len(REPLAYED) > 300
    wrong = []
    for entry, kv, rc, _ in REPLAYED:
        got = _call(entries[entry], ctx.h, entry, kv, a)
        if got != rc:
            wrong.append((ac.case_id((entry, kv, rc, 0)), "expected", rc, "got", got))
    assert not wrong, wrong


YARDSTICK_OF = {"conf_mix": "conf_copy", "bss_select": "bss_copy", "ptt_arbitrate": "ptt_copy", "link_watch": "link_copy", "jb_receive": "jb_copy",
                "plc_conceal": "plc_copy"}


@pytest.mark.parametrize("entry", sorted(YARDSTICK_OF))
def test_yardstick_rejects_what_its_twin_rejects(ctx, a, entry):
    """a yardstick takes its public entry's rule: every IGDSP_EINVAL row of the twin that launches nothing (at least three per stage),
    and the nothing-to-do rows, give the same code through the igdsp_internal_* entry.  (igdsp_internal_tx_copy has rows of its own
    above; rs, snd and tone: their own test files.)"""
    fn = capi.internal(YARDSTICK_OF[entry])
    rows = [c for c in REPLAYED if c[0] == entry]
    assert sum(1 for c in rows if c[2] == ac.EINVAL) >= 3
    wrong = [(ac.case_id(c), "got", got) for c in rows if (got := _call(fn, ctx.h, entry, c[1], a)) != c[2]]
    assert not wrong, wrong
