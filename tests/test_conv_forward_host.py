"""CPU: what the four forward entries of the hidden 3x3 convolution refuse (csrc/conv.hip: aurppo_conv3x3_f32, aurppo_conv3x3_pool_f32,
aurppo_conv3x3_planes_f32, aurppo_conv3x3_pool_planes_f32), row by row: the return code and the text of ``aurppo_last_error()``
equal tests/transcripts/conv_forward_refusals.json.  Every pointer is 0x1000 / 0x1004 and never dereferenced: each row is refused on the
host, without a device and so before any launch.  Rows with two defects pin which refusal is reported first.  One accepted call per
entry reaches the runtime, which has no device here: nothing more is refused than the table says.

The JSON is a RECORD OF THE LIBRARY AS IT WAS BEFORE the four entries were given one launcher: it was written by
``python tests/test_conv_forward_host.py`` against a build of that commit.  Re-record only when a refusal is meant to change, and READ
THE DIFF."""
import ctypes as C
import json
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import test_hip_ops_calls as TC             # noqa: E402

TRANSCRIPT = os.path.join(ROOT, "tests", "transcripts", "conv_forward_refusals.json")
EINVAL, ESHAPE, EHIP = -1, -2, -3
P, ODD = 0x1000, 0x1004          # a 16-byte aligned address and one that is not

# an entry's arguments in the order of its prototype (include/aurppo.h); "stream" is always null
ENTRIES = {
    "aurppo_conv3x3_f32": ("x", "w", "z", "B", "Ci", "Co", "H", "W", "pad", "mode", "ws"),
    "aurppo_conv3x3_pool_f32": ("x", "w", "bias", "z", "mask", "B", "Ci", "Co", "H", "W", "pad", "ws"),
    "aurppo_conv3x3_planes_f32": ("x", "w", "z", "B", "Ci", "Co", "H", "W", "pad", "ws"),
    "aurppo_conv3x3_pool_planes_f32": ("x", "x_is_planes", "w", "bias", "z", "mask", "yp", "B", "Ci", "Co", "H", "W", "pad", "ws"),
}
GOOD = dict(x=P, w=P, bias=P, z=P, mask=P, yp=P, ws=P, B=2, Ci=16, Co=32, H=8, W=8, pad=1, mode=0, x_is_planes=0)
# the ways to call them: (entry, what differs from GOOD).  "x" is the input, fp32 or planes, "z" the output (y of the pooled entries)
VARIANTS = {
    "f32/fwd": ("aurppo_conv3x3_f32", {}),
    "f32/dgrad": ("aurppo_conv3x3_f32", dict(mode=1, Ci=32, Co=16)),       # the product's input channels are Co
    "pool": ("aurppo_conv3x3_pool_f32", {}),
    "planes": ("aurppo_conv3x3_planes_f32", {}),
    "pool_planes/in": ("aurppo_conv3x3_pool_planes_f32", dict(x_is_planes=1, yp=0)),
    "pool_planes/out": ("aurppo_conv3x3_pool_planes_f32", dict(x_is_planes=0)),
    "pool_planes/in_out": ("aurppo_conv3x3_pool_planes_f32", dict(x_is_planes=1)),
    "pool_planes/neither": ("aurppo_conv3x3_pool_planes_f32", dict(x_is_planes=0, yp=0)),       # forwards to aurppo_conv3x3_pool_f32
}
POOLED = [v for v in VARIANTS if v.startswith("pool")]
DGRAD = "f32/dgrad"


def _rows():
    rows = {}

    def add(variant, what, **over):
        key = f"{variant}: {what}"
        assert key not in rows, key
        rows[key] = (variant, over)

    for v, (entry, base) in VARIANTS.items():
        names = ENTRIES[entry]
        cin = "Co" if v == DGRAD else "Ci"         # (mode 1 maps the filter's Co to the product's input channels)
        for ptr in ("x", "w", "z", "mask", "ws"):
            if ptr in names:
                add(v, f"null {ptr}", **{ptr: 0})
        add(v, "workspace off alignment", ws=ODD)
        if v in ("planes", "pool_planes/in", "pool_planes/in_out"):
            add(v, "input planes off alignment", x=ODD)
        if v in ("pool_planes/out", "pool_planes/in_out"):
            add(v, "output planes off alignment", yp=ODD)
            add(v, "Co 36 as planes", Co=36)
        if "mode" in names:
            add(v, "mode 2", mode=2)
        add(v, "pad -1", pad=-1)
        add(v, "pad 3", pad=3)
        for dim in ("B", "H", "W", "Ci", "Co"):
            add(v, f"{dim} 0", **{dim: 0})
        add(v, "input channels 24", **{cin: 24})
        # 1 x 1 under (the product's) padding 0: mode 1 pads by 2 - pad
        add(v, "empty output", H=1, W=1, pad=2 if v == DGRAD else 0)
        if v in POOLED:
            add(v, "no whole window", H=3, W=3, pad=0)
            add(v, "null mask + pad 3", mask=0, pad=3)
            add(v, "input channels 24 + no whole window", Ci=24, H=3, W=3, pad=0)
        add(v, "pad 3 + input channels 24", pad=3, **{cin: 24})
        add(v, "null x + pad 3", x=0, pad=3)
        add(v, "null w + pad 3", w=0, pad=3)
    add("f32/fwd", "mode 2 + null x", mode=2, x=0)
    add("pool_planes/in_out", "output planes off alignment + B 0", yp=ODD, B=0)
    add("pool_planes/out", "Co 36 as planes + no whole window", Co=36, H=3, W=3, pad=0)
    return rows


ROWS = _rows()


def _call(lib, variant, over):
    entry, base = VARIANTS[variant]
    a = dict(GOOD, **base)
    a.update(over)
    args = [C.c_void_p(a[n]) if isinstance(GOOD[n], int) and GOOD[n] == P else a[n] for n in ENTRIES[entry]]
    rc = getattr(lib, entry)(*args, None)
    return rc, lib.aurppo_last_error().decode()


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    return TC._lib.load()


def _recorded():
    with open(TRANSCRIPT) as f:
        return json.load(f)


def test_every_row_is_recorded_and_nothing_else():
    assert sorted(_recorded()) == sorted(ROWS)


def test_the_table_holds_what_it_should():
    """Single defects of every kind for every way to call the entries, and the two-defect rows that pin the order."""
    for v in VARIANTS:
        kinds = {k.split(": ", 1)[1] for k in ROWS if k.startswith(v + ": ")}
        assert {"null x", "null w", "null z", "null ws", "workspace off alignment", "pad -1", "pad 3", "B 0", "H 0", "W 0", "Ci 0", "Co 0",
                "input channels 24", "empty output", "pad 3 + input channels 24"} <= kinds, v
        assert ("null mask" in kinds) == ("no whole window" in kinds) == ("null mask + pad 3" in kinds) == (v in POOLED), v
        assert ("input channels 24 + no whole window" in kinds) == (v in POOLED)
    assert "planes: null x + pad 3" in ROWS and "pool_planes/in: null x + pad 3" in ROWS          # (null xp + bad pad)
    assert "f32/fwd: mode 2" in ROWS and "pool_planes/out: Co 36 as planes" in ROWS
    for code, _ in _recorded().values():
        assert code in (EINVAL, ESHAPE)          # a refusal, every one: no row reaches a launch


@pytest.mark.parametrize("key", sorted(ROWS))
def test_a_refused_call_returns_the_recorded_code_and_message(key, lib):
    variant, over = ROWS[key]
    want = _recorded()[key]
    assert want[0] in (EINVAL, ESHAPE)           # (asserted before the call: only a recorded refusal is ever sent to the library)
    assert list(_call(lib, variant, over)) == want


def test_a_refusal_names_the_entry_that_made_it():
    for key, (code, text) in _recorded().items():
        variant = key.split(": ", 1)[0]
        entry = "aurppo_conv3x3_pool_f32" if variant == "pool_planes/neither" else VARIANTS[variant][0]
        assert text.startswith(entry + ": "), key


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_an_accepted_call_without_a_device_fails_in_hip_not_before(variant, lib):
    """The other half of "refusals precede every launch": what is not refused reaches the runtime, which has no device here."""
    if torch.cuda.is_available():
        pytest.skip("needs a machine without a device")
    rc, text = _call(lib, variant, {})
    assert rc == EHIP, text
    rc, text = _call(lib, variant, dict(bias=0) if "bias" in ENTRIES[VARIANTS[variant][0]] else {})          # (a null bias is no defect)
    assert rc == EHIP, text


if __name__ == "__main__":
    import __graft_entry__ as g
    g.build()
    bound = TC._lib.load()
    result = {}
    for row_key in sorted(ROWS):
        code, text = _call(bound, *ROWS[row_key])
        result[row_key] = [code, text]
    os.makedirs(os.path.dirname(TRANSCRIPT), exist_ok=True)
    with open(TRANSCRIPT, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{len(result)} rows -> {TRANSCRIPT}")
