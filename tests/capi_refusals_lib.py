"""Replays the calls of tests/golden/capi_refusals.json against a loaded library (tests/golden/make_capi_refusals.py writes the
table with it, tests/test_capi_refusals_cpu.py checks the tree's library against it).

The table holds one set of good argument values by parameter name ("good", with a symbol's own where they differ), the
faults - [name, changes to the good values]; a change names a parameter, or "parameter.k" for field k of a struct - and per
symbol its parameter names, its cases - [fault, return code, message, outs] - and its pairs - [case i, case j, return code,
message, outs]: the faults of the symbol's cases i and j at once.  `fault`, `message` and `outs` index the table's lists of
faults, of svs_last_error() texts and of the values the out parameters hold after the call, in argument order.

A number or null is passed as it is (pointers are fake addresses: no case gets as far as reading one); what the library does
read is built: planes, order, dither ([key, first_frame, reserved]), coeffs ([count, index...]) and counts as structs by
reference, {"u32s": [..]} as an array of uint32 (colour weights), ascii as a character payload, n_embedded and n_bits_out as
uint64 out parameters pre-set to the value, {"filled": [n, byte]} as a real array of n bytes pre-set to `byte` that the call
may write (the tally and the counts of the host soft calls); its contents after the call are recorded among the outs, as
"<n>x<byte>" while all its bytes are equal and in hex otherwise."""
import ctypes as C

from svsdct import native

SENTINEL = 0xDEADBEEFCAFEF00D
STRUCTS = ("planes", "order", "coeffs", "dither", "ascii", "counts")
U64_OUTS = ("n_embedded", "n_bits_out")


def arguments(parameters, good, changes):
    """the argument list of a call: the good values with `changes` applied, each wrapped into the form _build takes"""
    v = {k: (list(x) if isinstance(x, list) else x) for k, x in good.items()}
    for where, value in changes.items():
        name, _, field = where.partition(".")
        if field:
            v[name][int(field)] = value
        else:
            v[name] = value
    wrap = lambda a, x: x if x is None else {a: x} if a in STRUCTS else {"u64": x} if a in U64_OUTS else x   # noqa: E731
    return [wrap(a, v[a]) for a in parameters]


def cases_of(table, symbol):
    """-> (name, arguments, return code, message text, outs) of every case and pair of the symbol"""
    entry = table["symbols"][symbol]
    good = {**table["good"], **entry["good"]}
    singles = [(*table["faults"][f], *r) for f, *r in entry["cases"]]
    both = [(f"{singles[i][0]} + {singles[j][0]}", {**singles[i][1], **singles[j][1]}, *r) for i, j, *r in entry["pairs"]]
    for name, changes, rc, message, outs in singles + both:
        yield name, arguments(entry["parameters"], good, changes), rc, table["messages"][message], table["outs"][outs]


def _build(arg):
    """-> (what to pass, the ctypes object to keep alive and read back or None, is an out parameter)"""
    if not isinstance(arg, dict):
        return arg, None, False
    (kind, v), = arg.items()
    if kind == "planes":
        obj = native.Planes(*v)
    elif kind == "order":
        obj = native.BlockOrder(*v)
    elif kind == "dither":
        obj = native.Dither(*v)
    elif kind == "coeffs":
        obj = native.Coeffs()
        obj.count = v[0]
        for i, k in enumerate(v[1:]):
            obj.index[i] = k
    elif kind == "u32s":
        obj = (C.c_uint32 * len(v))(*v)
        return C.cast(obj, C.c_void_p), obj, False
    elif kind == "ascii":
        obj = C.create_string_buffer(v.encode("ascii"))
        return C.cast(obj, C.c_void_p), obj, False
    elif kind == "u64":
        obj = C.c_uint64(v)
        return C.byref(obj), obj, True
    elif kind == "filled":
        obj = (C.c_uint8 * v[0])(*([v[1]] * v[0]))
        return C.cast(obj, C.c_void_p), obj, True
    elif kind == "counts":
        obj = native.ReadbackCounts(*v)
        return C.byref(obj), obj, True
    else:
        raise ValueError(f"unknown argument kind {kind!r}")
    return C.byref(obj), obj, False


def _read_out(o):
    if isinstance(o, native.ReadbackCounts):
        return [int(o.repaired), int(o.unrepaired)]
    if isinstance(o, C.Array):
        b = bytes(o)
        return f"{len(b)}x{b[0]:02x}" if b == b[:1] * len(b) else b.hex()
    return int(o.value)


def run_case(lib, symbol, args):
    """-> (return code, svs_last_error() text ("" for SVS_OK), the out parameters' values after the call)"""
    built = [_build(a) for a in args]
    rc = getattr(lib, symbol)(*[b[0] for b in built])
    outs = [_read_out(o) for _, o, is_out in built if is_out]
    return rc, "" if rc == native.SVS_OK else lib.svs_last_error().decode("utf-8"), outs
