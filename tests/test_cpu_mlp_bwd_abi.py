"""CPU tests of the shared-MLP backward boundary (ABI 21): the four argument structs of include/gspn_hip.h against their ctypes mirrors, the
three launchers that take them against the binding table, and the argument checks of the one pass-B entry point, which return before any
HIP call."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARG, UNSUPPORTED = -1, -2


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gspn_hip.h")).read(), flags=re.S)


def _ctype(decl, structs):
    """the ctypes type of one C declarator `[const] type[*] name`: device pointers are void*, a writable `int*` is a count the launcher
    hands back on the host"""
    kind = decl.replace("const ", "").replace("struct ", "").replace("*", " * ").split()
    if "*" not in kind:
        return {"int": ctypes.c_int, "long": ctypes.c_long, "float": ctypes.c_float, "double": ctypes.c_double}[kind[0]]
    if kind[0] in structs:
        return ctypes.POINTER(structs[kind[0]])
    return ctypes.POINTER(ctypes.c_int) if (kind[0] == "int" and "const" not in decl) else ctypes.c_void_p


def test_header_structs_and_launchers_match_the_binding():
    from gspn_amd import _lib
    code = _header()
    structs = {"gspn_dy_args": _lib.DyArgs, "gspn_gather_args": _lib.GatherArgs, "gspn_dw_args": _lib.DwArgs, "gspn_rsum_args": _lib.RsumArgs}
    for name, mirror in structs.items():
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), code, flags=re.S).group(1)
        fields = [f.strip() for f in body.split(";") if f.strip()]
        declared = [(f.replace("*", " ").split()[-1], _ctype(f, {})) for f in fields]
        assert declared == list(mirror._fields_), name
    assert len(_lib.DwArgs._fields_) == 13 and len(_lib.RsumArgs._fields_) == 9
    for name in ("gspn_mlp_bwd_data", "gspn_mlp_bwd_dw", "gspn_mlp_bwd_data_pooltop"):
        args = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, code).group(1).split(",")
        assert [_ctype(a.strip(), structs) for a in args] == _lib.SIGNATURES[name], name
    for gone in ("gspn_mlp_bwd_data_cols", "gspn_mlp_bwd_data_dw", "gspn_mlp_bwd_data_dw2", "gspn_mlp_bwd_data_ex"):
        assert gone not in _lib.SIGNATURES and not re.search(r"\b%s\b" % gone, code)
    assert re.search(r"^ \*\s+21: gspn_dw_args / gspn_rsum_args", open(os.path.join(ROOT, "include", "gspn_hip.h")).read(), flags=re.M)


# ---- the merged checker -------------------------------------------------------------------------------------------------------------
# A call is described by plain values: the scalars, `a`, `dw` and `rs` as dicts of field values (None: a NULL struct), pointers as small
# non-zero integers that nothing dereferences (every check returns before the first HIP call).  GOOD is a complete call with both jobs; a
# case is GOOD with a few values replaced.  Expected: what the entry point that took the same arguments before ABI 21 returned, obtained
# by running this table once against the library of the commit before (gspn_mlp_bwd_data_cols for the plain form, gspn_mlp_bwd_data_dw2
# where a second job is given, gspn_mlp_bwd_data_dw for a job without `work`, gspn_mlp_bwd_data_ex for everything else).
P = 0x1000
GOOD_A = dict(Y=P, ldy=20, dZ=P, ldz=20, dPool=0, pool_arg=0, ns=0, scale=P, shift=P, cA=P, cB=P, cC=P)
GOOD_DW = dict(X=P, ldx=24, var=P, gamma=P, eps=1e-3, use_bn=1, is_training=1, work=P, dW=P, part2=0, cin2=0, nslots2=0, dW2=0)
GOOD_RS = dict(Yp=P, ldyp=24, scale=P, shift=P, mean=P, var=P, eps=1e-3, part=P, nparts_out=True)
GOOD = dict(rows=2080, cin=24, cout=20, col0=0, ncols=24, ldx=24)
PLAIN, DW, RS, BOTH = (False, False), (True, False), (False, True), (True, True)

CASES = [
    # (what, form, changes to the scalars, to a, to dw, to rs, expected)
    ("NULL a", BOTH, {}, None, {}, {}, ARG),
    ("NULL a, plain", PLAIN, {}, None, {}, {}, ARG),
    ("a without Y", PLAIN, {}, dict(Y=0), {}, {}, ARG),
    ("a without scale", DW, {}, dict(scale=0), {}, {}, ARG),
    ("a without shift", RS, {}, dict(shift=0), {}, {}, ARG),
    ("a without cA", PLAIN, {}, dict(cA=0), {}, {}, ARG),
    ("a without cB", DW, {}, dict(cB=0), {}, {}, ARG),
    ("a without cC", BOTH, {}, dict(cC=0), {}, {}, ARG),
    ("a without an upstream gradient", PLAIN, {}, dict(dZ=0), {}, {}, ARG),
    ("pooled a without pool_arg", BOTH, {}, dict(dZ=0, dPool=P, ns=32), {}, {}, ARG),
    ("pooled a with ns = 0", PLAIN, {}, dict(dZ=0, dPool=P, pool_arg=P), {}, {}, ARG),
    ("col0 + ncols > cin", PLAIN, dict(col0=4, ncols=21), {}, {}, {}, ARG),
    ("col0 + ncols > cin, dw", DW, dict(col0=4, ncols=21), {}, {}, {}, ARG),
    ("col0 < 0", PLAIN, dict(col0=-1, ncols=4), {}, {}, {}, ARG),
    ("ncols == 0", DW, dict(ncols=0), {}, {}, {}, ARG),
    ("ldx < cin", PLAIN, dict(ldx=23), {}, {}, {}, ARG),
    ("ldx < cin, both", BOTH, dict(ldx=23), {}, {}, {}, ARG),
    ("cin == 0", PLAIN, dict(cin=0, ncols=0, ldx=0), {}, {}, {}, ARG),
    ("cout == 0", RS, dict(cout=0), {}, {}, {}, ARG),
    ("rows == 0, plain: nothing to do", PLAIN, dict(rows=0), {}, {}, {}, 0),
    ("rows == 0, dw", DW, dict(rows=0), {}, {}, {}, ARG),
    ("rows == 0, rs", RS, dict(rows=0), {}, {}, {}, ARG),
    ("rows == 0, both", BOTH, dict(rows=0), {}, {}, {}, ARG),
    ("rows < 0, plain", PLAIN, dict(rows=-128), {}, {}, {}, ARG),
    ("rows < 0, dw", DW, dict(rows=-128), {}, {}, {}, ARG),
    ("rows < 0, rs", RS, dict(rows=-128), {}, {}, {}, ARG),
    ("rows < 0, both", BOTH, dict(rows=-128), {}, {}, {}, ARG),
    ("cin > MAXCH, plain", PLAIN, dict(cin=1028, ncols=1028, ldx=1028), {}, {}, {}, UNSUPPORTED),
    ("cin > MAXCH, both", BOTH, dict(cin=1028, ncols=1028, ldx=1028), {}, dict(ldx=1028), dict(ldyp=1028), UNSUPPORTED),
    ("cout > MAXCH, dw", DW, dict(cout=1028), {}, {}, {}, UNSUPPORTED),
    ("rows >= 2^31", PLAIN, dict(rows=1 << 31), {}, {}, {}, UNSUPPORTED),
    ("rows >= 2^31, both", BOTH, dict(rows=1 << 31), {}, {}, {}, UNSUPPORTED),
    ("cin > MAXCH beats a defective dw", DW, dict(cin=1028, ncols=1028, ldx=1028), {}, dict(dW=0), {}, UNSUPPORTED),
    ("dw without work", DW, {}, {}, dict(work=0), {}, ARG),
    ("dw without dW", DW, {}, {}, dict(dW=0), {}, ARG),
    ("dw without dW, both", BOTH, {}, {}, dict(dW=0), {}, ARG),
    ("dw: use_bn without var", DW, {}, {}, dict(var=0), {}, ARG),
    ("dw: use_bn without var, both", BOTH, {}, {}, dict(var=0), {}, ARG),
    ("dw: X with ldx < cin", DW, {}, {}, dict(ldx=23), {}, ARG),
    ("dw: X with ldx < cin, both", BOTH, {}, {}, dict(ldx=23), {}, ARG),
    ("rs with col0 != 0", RS, dict(col0=4, ncols=20), {}, {}, {}, ARG),
    ("rs with ncols != cin", BOTH, dict(ncols=20), {}, {}, {}, ARG),
    ("rs without nparts_out", RS, {}, {}, {}, dict(nparts_out=False), ARG),
    ("rs without nparts_out, both", BOTH, {}, {}, {}, dict(nparts_out=False), ARG),
    ("rs without Yp", RS, {}, {}, {}, dict(Yp=0), ARG),
    ("rs with ldyp < cin", BOTH, {}, {}, {}, dict(ldyp=23), ARG),
    ("rs without scale", RS, {}, {}, {}, dict(scale=0), ARG),
    ("rs without shift", RS, {}, {}, {}, dict(shift=0), ARG),
    ("rs without mean", RS, {}, {}, {}, dict(mean=0), ARG),
    ("rs without var", BOTH, {}, {}, {}, dict(var=0), ARG),
    ("cin2 > 0 without part2", DW, {}, {}, dict(cin2=3, nslots2=8, dW2=P), {}, ARG),
    ("cin2 > 0 without dW2", DW, {}, {}, dict(cin2=3, nslots2=8, part2=P), {}, ARG),
    ("cin2 > 0 without slots", DW, {}, {}, dict(cin2=3, part2=P, dW2=P), {}, ARG),
    ("cin2 < 0", DW, {}, {}, dict(cin2=-1, nslots2=8, part2=P, dW2=P), {}, ARG),
    ("nslots2 < 0", DW, {}, {}, dict(nslots2=-1), {}, ARG),
    ("a second job on a defective first", DW, {}, {}, dict(cin2=3, nslots2=8, part2=P, dW2=P, work=0), {}, ARG),
]


def build_call(case):
    """(scalars, a, dw, rs) of a case as dicts (a / dw / rs None where the struct is NULL)"""
    _, (with_dw, with_rs), ch_s, ch_a, ch_dw, ch_rs, _ = case
    a = None if ch_a is None else dict(GOOD_A, **ch_a)
    return dict(GOOD, **ch_s), a, dict(GOOD_DW, **ch_dw) if with_dw else None, dict(GOOD_RS, **ch_rs) if with_rs else None


def test_every_listed_defect_is_in_the_table():
    what = " | ".join(c[0] for c in CASES)
    for needle in ("NULL a", "without cA", "without cB", "without cC", "col0 + ncols > cin", "ldx < cin", "rows == 0, plain", "rows == 0, dw", "rows == 0, rs",
                   "rows == 0, both", "rows < 0", "cin > MAXCH", "dw without work", "dw without dW", "use_bn without var", "rs with col0 != 0",
                   "rs without nparts_out", "cin2 > 0 without part2"):
        assert needle in what, needle
    assert len({c[0] for c in CASES}) == len(CASES)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_merged_pass_b_checker_returns_what_the_removed_entry_points_returned(case):
    from gspn_amd import _lib as L
    lib = L.lib()
    s, a, dw, rs = build_call(case)
    npart = ctypes.c_int(-7)
    sa = L.DyArgs(**a) if a is not None else None
    sdw = L.DwArgs(**dw) if dw is not None else None
    srs = None
    if rs is not None:
        srs = L.RsumArgs(**dict(rs, nparts_out=ctypes.pointer(npart) if rs["nparts_out"] else None))
    rc = lib.gspn_mlp_bwd_data(s["rows"], s["cin"], s["cout"], ctypes.byref(sa) if sa is not None else None, ctypes.c_void_p(P), s["col0"], s["ncols"],
                               ctypes.c_void_p(P), s["ldx"], ctypes.byref(sdw) if sdw is not None else None,
                               ctypes.byref(srs) if srs is not None else None, None)
    assert rc == case[-1]
    assert npart.value == -7                     # a rejected call writes nothing
