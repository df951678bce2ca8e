"""vafc_corr.hip at double precision: the correlation kernels against a plain
statement of correlation-matrix.c:94-162, bit for bit, over the tile grid
(TA = 32 lower x TB = 64 higher samples), the CH = 64 row chunks, the 32-row
validity words, ragged row counts and "nan"/"inf" rows.

Two forms of the statement, both row by row in the reference's order with
every operation rounded on its own:
  statement()    numpy, one vector element per pair i < j (the expected value
                 of everything finite);
  scalar_pair()  Python floats, one pair, every operation's NaN chosen the
                 x86 way (first operand if a NaN, else the second, else the
                 negative default NaN) -- the sign the reference prints.
statement(x86=True) applies the same NaN rule, so the two forms can be held
against each other on non-finite sets as well.

CPU tests pin both forms to the recorded reference outputs (the goldens) and,
on generated sets, to oracle/corr_oracle.c (itself pinned to the reference by
test_corr.py::test_oracle_matches_reference).  GPU tests compare
vafc.correlation_matrix_raw with the statement as uint64 views."""
import functools
import math
import os
import struct
import subprocess

import numpy as np
import pytest

from test_corr import CASES, CORR, ORACLE, case_options

TA, TB, CH = 32, 64, 64          # vafc_corr.hip's tile and chunk sizes (the shapes below sit on their edges)

POS_NAN = struct.unpack("<d", struct.pack("<Q", 0x7FF8000000000000))[0]
NEG_NAN = struct.unpack("<d", struct.pack("<Q", 0xFFF8000000000000))[0]   # x86's default NaN


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


# --- the statement, vectorised over pairs ------------------------------------

def _nanfix(r, a, b):
    return np.where(np.isnan(r), np.where(np.isnan(a), a, np.where(np.isnan(b), b, NEG_NAN)), r)


def statement(vaf, dep, ns, min_snps, min_depth, x86=False):
    """correlation-matrix.c:94-162 for every pair i < j at once.  vaf/dep are
    [n][stride], sample s has ns[s] rows (what lies past them is never read).
    Returns the pair index vectors I, J, the intermediate values (cnt, the
    valid-row count per 32-row word wcnt, sx, sy, mx, my, sxy, sxx, syy, the
    epsilon-branch mask eps) and the results r, all per pair."""
    vaf = np.asarray(vaf, np.float64)
    dep = np.asarray(dep, np.int64)
    ns = np.asarray(ns, np.int64)
    n, stride = vaf.shape
    I, J = np.triu_indices(n, 1)
    inside = np.arange(stride)[None, :] < ns[:, None]
    xe = np.where(inside, vaf, 0.0)                       # past a sample's end: vaf 0.0 ...
    de = np.where(inside, dep, 0)                         # ... depth 0 (the higher sample of a pair)
    ok_lo = (inside & (dep >= min_depth)).T.copy()        # the lower sample bounds the row range
    ok_hi = (de >= min_depth).T.copy()
    xt = xe.T.copy()
    if x86:
        add = lambda a, b: _nanfix(a + b, a, b)
        sub = lambda a, b: _nanfix(a - b, a, b)
        mul = lambda a, b: _nanfix(a * b, a, b)
        div = lambda a, b: _nanfix(a / b, a, b)
        sqrt = lambda a: np.where(np.isnan(a), a, np.sqrt(a))
    else:
        add, sub, mul, div, sqrt = np.add, np.subtract, np.multiply, np.divide, np.sqrt
    R = int(ns.max()) if n else 0
    z = np.zeros(len(I))
    cnt = np.zeros(len(I), np.int64)
    wcnt = np.zeros((len(I), (R + 31) // 32), np.int64)
    sx, sy = z.copy(), z.copy()
    with np.errstate(all="ignore"):
        for r in range(R):
            valid = ok_lo[r][I] & ok_hi[r][J]
            cnt = np.where(valid, cnt + 1, cnt)
            wcnt[:, r // 32] += valid
            sx = np.where(valid, add(sx, xt[r][I]), sx)
            sy = np.where(valid, add(sy, xt[r][J]), sy)
        c = np.maximum(cnt, 1).astype(np.float64)
        mx = np.where(cnt > 0, div(sx, c), 0.0)          # unused when no row is valid
        my = np.where(cnt > 0, div(sy, c), 0.0)
        sxy, sxx, syy = z.copy(), z.copy(), z.copy()
        for r in range(R):
            valid = ok_lo[r][I] & ok_hi[r][J]
            dx = sub(xt[r][I], mx)
            dy = sub(xt[r][J], my)
            sxy = np.where(valid, add(sxy, mul(dx, dy)), sxy)
            sxx = np.where(valid, add(sxx, mul(dx, dx)), sxx)
            syy = np.where(valid, add(syy, mul(dy, dy)), syy)
        da, db = sqrt(sxx), sqrt(syy)
        eps = (da < 1e-10) | (db < 1e-10)
        r_eps = div(sxy, add(sqrt(mul(sxx, syy)), 0.00001))
        r_std = div(sxy, mul(db, da))
        res = np.where(cnt < min_snps, 0.0, np.where(eps, r_eps, r_std))
    return dict(I=I, J=J, cnt=cnt, wcnt=wcnt, sx=sx, sy=sy, mx=mx, my=my, sxy=sxy, sxx=sxx, syy=syy, eps=eps,
                r=res)


def matrix(st, n):
    m = np.eye(n)
    m[st["I"], st["J"]] = st["r"]
    m[st["J"], st["I"]] = st["r"]
    return m


# --- the statement, one pair, x86 NaNs spelled out ---------------------------

def _x86(r, a, b):
    """The result of an SSE add/sub/mul/div of (a, b) whose value is r."""
    if r == r:
        return r
    if a != a:
        return a
    if b != b:
        return b
    return NEG_NAN


def _sqrt(a):
    if a != a:
        return a
    return math.sqrt(a) if a >= 0 else NEG_NAN


def scalar_pair(xa, da, xb, db, n, min_snps, min_depth):
    """One pair over rows [0, n); xb/db already read 0.0 / 0 past the higher
    sample's end.  Operand order of correlation-matrix.c:108-125 as compiled:
    sum + x, x - mean, dx * dy, sum + product, sum / count."""
    ok = [da[r] >= min_depth and db[r] >= min_depth for r in range(n)]
    cnt = sum(ok)
    if cnt < min_snps:
        return 0.0
    sx = sy = 0.0
    for r in range(n):
        if ok[r]:
            sx = _x86(sx + xa[r], sx, xa[r])
            sy = _x86(sy + xb[r], sy, xb[r])
    c = float(cnt)
    mx = _x86(sx / c, sx, c) if cnt else 0.0
    my = _x86(sy / c, sy, c) if cnt else 0.0
    sxy = sxx = syy = 0.0
    for r in range(n):
        if ok[r]:
            dx = _x86(xa[r] - mx, xa[r], mx)
            dy = _x86(xb[r] - my, xb[r], my)
            p, q, u = _x86(dx * dy, dx, dy), _x86(dx * dx, dx, dx), _x86(dy * dy, dy, dy)
            sxy = _x86(sxy + p, sxy, p)
            sxx = _x86(sxx + q, sxx, q)
            syy = _x86(syy + u, syy, u)
    ex, ey = _sqrt(sxx), _sqrt(syy)
    if ex < 1e-10 or ey < 1e-10:
        s = _sqrt(_x86(sxx * syy, sxx, syy))
        e = _x86(s + 0.00001, s, 0.00001)
        return _x86(sxy / e, sxy, e)
    d = _x86(ey * ex, ey, ex)
    return _x86(sxy / d, sxy, d)


def scalar_pairs(vaf, dep, ns, min_snps, min_depth, pairs):
    n, stride = vaf.shape
    inside = np.arange(stride)[None, :] < np.asarray(ns)[:, None]
    xe = np.where(inside, vaf, 0.0).tolist()
    de = np.where(inside, dep, 0).tolist()
    return np.array([scalar_pair(xe[i], de[i], xe[j], de[j], int(ns[i]), min_snps, min_depth) for i, j in pairs],
                    np.float64)


def scalar_matrix(vaf, dep, ns, min_snps, min_depth):
    n = len(ns)
    I, J = np.triu_indices(n, 1)
    return matrix(dict(I=I, J=J, r=scalar_pairs(vaf, dep, ns, min_snps, min_depth, zip(I.tolist(), J.tolist()))), n)


# --- text --------------------------------------------------------------------

def fmt(v):
    """printf("%.6f"): a NaN prints by its sign bit."""
    if v != v:
        return "-nan" if math.copysign(1.0, v) < 0 else "nan"
    return "%.6f" % v


def corr_text(names, m):
    out = ["Sample" + "".join("\t" + s for s in names)]
    for i, s in enumerate(names):
        out.append(s + "".join("\t" + fmt(float(v)) for v in m[i]))
    return "\n".join(out) + "\n"


def parse_vaf(tok):
    """strtod on the fixtures' VAF column."""
    t = tok.lower()
    if t.lstrip("+-") == "nan":
        return NEG_NAN if t.startswith("-") else POS_NAN
    return float(tok)


def vaf_token(v, finite_fmt):
    if v != v:
        return "-nan" if math.copysign(1.0, v) < 0 else "nan"
    if math.isinf(v):
        return "inf" if v > 0 else "-inf"
    return finite_fmt % v


def write_set(d, vaf, dep, ns, finite_fmt="%.4f"):
    """The set as .vaf files whose text reads back as exactly these doubles."""
    paths = []
    for s in range(vaf.shape[0]):
        p = os.path.join(d, "k%03d.vaf" % s)
        lines = ["# Average depth: 1.00\n", "CHR\tPOS\tRSID\tREF\tALT\tREF_COUNT\tALT_COUNT\tTOTAL_COUNT\tVAF\n"]
        for i in range(int(ns[s])):
            tok = vaf_token(float(vaf[s, i]), finite_fmt)
            back = parse_vaf(tok)
            assert struct.pack("<d", back) == struct.pack("<d", float(vaf[s, i])), (s, i, tok)
            lines.append("chr1\t%d\trs%d\tA\tC\t0\t0\t%d\t%s\n" % (i, i, dep[s, i], tok))
        with open(p, "w") as f:
            f.write("".join(lines))
        paths.append(p)
    return paths, ["k%03d" % s for s in range(vaf.shape[0])]


def oracle_text(tmp, paths, min_snps, min_depth):
    o = os.path.join(tmp, "orc.corr")
    p = subprocess.run([ORACLE, "-o", o, "-m", str(min_snps), "-d", str(min_depth)] + paths, capture_output=True,
                       timeout=120)
    assert p.returncode == 0, p.stderr
    with open(o) as f:
        return f.read()


# --- generated sets ----------------------------------------------------------

GEOMETRY = [(2, 1, 0, 0),          # smallest input
            (33, 31, 20, 1),       # second a tile, one partial word
            (65, 64, 5, 10),       # second b tile, exactly one chunk
            (66, 65, 1, -3),       # one row into a second chunk, negative depth bound
            (97, 129, 20, 1),      # tile (a0 = 64, b0 = 64) on the diagonal, exit tile (a0 = 96, b0 = 0)
            (129, 33, 0, 0),       # third b tile of one column
            (193, 257, 3, 2)]      # 4 x 7 tiles, five chunks
CONST, TWIN_A, TWIN_B, BOUND_ALL, BOUND_AT, BOUND_BELOW = 3, 4, 5, 16, 17, 18
WAVE = slice(8, 16)                # one wave's eight a rows of the first tile


def base_set(rng, n, R):
    """VAFs on the %.4f grid around four genotype vectors; depths mostly well
    above every bound used here, some 0, some negative, some low."""
    g = rng.integers(0, 3, (4, R))
    vaf = np.clip(g[rng.integers(0, 4, n)] * 5000 + rng.integers(-400, 401, (n, R)), 0, 10000) / 10000.0
    u = rng.random((n, R))
    dep = rng.integers(12, 61, (n, R))
    dep = np.where(u < 0.05, 0, dep)
    dep = np.where((u >= 0.05) & (u < 0.10), rng.integers(-6, 0, (n, R)), dep)
    dep = np.where((u >= 0.10) & (u < 0.15), rng.integers(1, 10, (n, R)), dep)
    return vaf, dep.astype(np.int32)


def fill_stride_area(vaf, dep, ns):
    inside = np.arange(vaf.shape[1])[None, :] < np.asarray(ns)[:, None]
    vaf[~inside] = np.nan
    dep[~inside] = 1000


@functools.lru_cache(maxsize=None)
def geometry_set(n, R, min_snps, min_depth):
    """(vaf, dep, ns, statement) of one shape; computed once, never modified."""
    rng = np.random.default_rng(n * 1000 + R)
    if n == 2:
        vaf, dep = np.array([[0.3], [0.7]]), np.array([[5], [7]], np.int32)
        ns = np.array([1, 0], np.int32)
    else:
        # a depth that no bound used here admits: 0 where min_depth > 0 (the
        # words below are then empty, not rows of valid zeros)
        dead = min(0, min_depth - 1)
        vaf, dep = base_set(rng, n, R)
        ns = np.full(n, R, np.int32)
        ns[1], ns[2] = 1, 0
        vaf[CONST], dep[CONST] = 0.25, 30
        vaf[TWIN_B], dep[TWIN_B] = vaf[TWIN_A], dep[TWIN_A]
        if min_snps > 0:
            live = np.array([r for r in range(R) if not 32 <= r < 64])
            pick = live[np.linspace(0, len(live) - 1, min_snps).astype(int)]
            assert len(set(pick.tolist())) == min_snps
            dep[BOUND_ALL] = 30
            dep[BOUND_AT], dep[BOUND_BELOW] = dead, dead
            dep[BOUND_AT, pick] = 30
            dep[BOUND_BELOW, pick[:-1]] = 30
        dep[:, 32:64] = dead                               # a word that is empty for every wave
        dep[WAVE, 64:96] = dead                            # ... and one that is empty for one wave only
        lens = [R - 1, 33, 65, R // 2, 31, 64, 2]
        for k in range((n + TA - 1) // TA):                # a short sample in every tile row
            ns[min(TA * k + 6, n - 1)] = max(1, min(R - 1, lens[k % len(lens)]))
        if ns[n - 1] == R:
            ns[n - 1] = R // 2 + 1
    fill_stride_area(vaf, dep, ns)
    for a in (vaf, dep, ns):
        a.setflags(write=False)
    return vaf, dep, ns, statement(vaf, dep, ns, min_snps, min_depth)


def check_geometry_content(n, R, min_snps, min_depth):
    """What the issue wants in every set, read off the statement's own values."""
    vaf, dep, ns, st = geometry_set(n, R, min_snps, min_depth)
    I, J, cnt, r = st["I"], st["J"], st["cnt"], st["r"]
    inside = np.arange(R)[None, :] < ns[:, None]
    assert np.isfinite(r).all()                            # nothing saw the stride area
    assert (~inside).any() and np.isnan(vaf[~inside]).all() and (dep[~inside] == 1000).all()
    assert {0, 1, R} <= set(ns.tolist())
    if n == 2:
        assert (ns[I] > ns[J]).any()
        return
    assert (ns[I] < ns[J]).any() and (ns[I] > ns[J]).any()
    for k in range((n + TA - 1) // TA):
        assert (ns[TA * k:TA * (k + 1)] < R).any(), k
    assert (dep[inside] == 0).any() and (dep[inside] < 0).any()
    if R > 32:
        assert (st["wcnt"][:, 1] == 0).all()
    if R > 64:
        w = st["wcnt"][:, 2]
        in_wave = (I >= WAVE.start) & (I < WAVE.stop)
        assert (w[in_wave] == 0).all()
        assert (w[(I < WAVE.start) & (J < TB)] > 0).any() and (w[(I >= WAVE.stop) & (I < TA) & (J < TB)] > 0).any()
    of_const = (I == CONST) | (J == CONST)
    assert of_const.sum() == n - 1 and st["eps"][of_const].all()
    twin = np.flatnonzero((I == TWIN_A) & (J == TWIN_B))[0]
    assert cnt[twin] >= max(min_snps, 2) and r[twin] != 0.0
    assert bits(st["sxx"])[twin] == bits(st["syy"])[twin] == bits(st["sxy"])[twin]
    if min_snps > 0:
        at = np.flatnonzero((I == BOUND_ALL) & (J == BOUND_AT))[0]
        below = np.flatnonzero((I == BOUND_ALL) & (J == BOUND_BELOW))[0]
        assert cnt[at] == min_snps and cnt[below] == min_snps - 1
        assert (bits(r)[cnt < min_snps] == 0).all()
    assert 2 * int(((r != 0.0) & np.isfinite(r)).sum()) >= len(r)


KINDS = (POS_NAN, NEG_NAN, math.inf, -math.inf)
NF_SHAPE = (70, 130, 5)            # samples, rows, min_snps: two b tiles, three a tiles


@functools.lru_cache(maxsize=None)
def nonfinite_set(min_depth):
    """70 x 130 with nan / -nan / inf / -inf in rows that are valid for their
    pairs, that the sample's own depth excludes, that only the partner's depth
    excludes, and that lie past the lower sample's end; in every tile."""
    n, R, min_snps = NF_SHAPE
    dead = min(0, min_depth - 1)
    rng = np.random.default_rng(70130)
    vaf, dep = base_set(rng, n, R)
    ns = np.full(n, R, np.int32)
    ns[5], ns[37], ns[66], ns[69] = 40, 70, 100, 20
    # (sample, row, value, own depth): own depth 30 = valid unless the partner excludes the row
    own_valid = [(2, 10, 0), (10, 33, 1), (35, 64, 2), (40, 100, 3), (65, 7, 0), (67, 127, 2), (30, 100, 3),
                 (69, 19, 1)]
    own_excluded = [(7, 3, 2), (20, 65, 1), (45, 129, 3), (68, 31, 0), (1, 77, 2), (66, 99, 1)]
    partner_only = [(12, 50, 2, (13, 14, 33, 50, 66)), (48, 90, 1, (3, 49, 64, 9)), (64, 12, 3, (0, 36, 68)),
                    (33, 115, 0, (34, 65, 6))]
    for s, r, k in own_valid:
        vaf[s, r], dep[s, r] = KINDS[k], 30
    for s, r, k in own_excluded:
        vaf[s, r], dep[s, r] = KINDS[k], dead
    for s, r, k, partners in partner_only:
        vaf[s, r], dep[s, r] = KINDS[k], 30
        dep[list(partners), r] = dead
    fill_stride_area(vaf, dep, ns)
    zeroed = np.where(np.isfinite(vaf), vaf, 0.0)
    fill_stride_area(zeroed, dep, ns)
    for a in (vaf, dep, ns, zeroed):
        a.setflags(write=False)
    st = statement(vaf, dep, ns, min_snps, min_depth)
    st0 = statement(zeroed, dep, ns, min_snps, min_depth)
    I, J = st["I"], st["J"]
    # where each pair meets the non-finite values that are stored inside a sample
    inside = np.arange(R)[None, :] < ns[:, None]
    nf = ~np.isfinite(vaf) & inside
    de = np.where(inside, dep, 0)
    z = np.zeros(len(I), bool)
    cls = dict(valid=z.copy(), own=z.copy(), partner=z.copy(), past=z.copy())
    for r in np.flatnonzero(nf.any(axis=0)):
        A, B, inr = nf[I, r], nf[J, r], r < ns[I]
        oka, okb = inr & (dep[I, r] >= min_depth), de[J, r] >= min_depth
        cls["valid"] |= oka & okb & (A | B)
        cls["own"] |= (A & inr & ~oka) | (B & ~okb)
        cls["partner"] |= (A & oka & ~okb) | (B & okb & inr & ~oka)
        cls["past"] |= B & ~inr
    kind2 = cls["valid"]
    kind1 = (cls["own"] | cls["partner"] | cls["past"]) & ~kind2
    pairs2 = list(zip(I[kind2].tolist(), J[kind2].tolist()))
    want2 = scalar_pairs(vaf, dep, ns, min_snps, min_depth, pairs2)
    return dict(vaf=vaf, dep=dep, ns=ns, zeroed=zeroed, st=st, st0=st0, cls=cls, kind1=kind1, kind2=kind2,
                want2=want2)


def check_nonfinite_content(min_depth):
    S = nonfinite_set(min_depth)
    n, R, min_snps = NF_SHAPE
    I, J, cls, kind1, kind2 = S["st"]["I"], S["st"]["J"], S["cls"], S["kind1"], S["kind2"]
    inside = np.arange(R)[None, :] < S["ns"][:, None]
    stored = bits(S["vaf"])[~np.isfinite(S["vaf"]) & inside]
    assert set(stored.tolist()) == set(bits(np.array(KINDS)).tolist())
    assert kind1.sum() >= 10 and kind2.sum() >= 10
    assert (kind1 & cls["own"]).any() and (kind1 & cls["past"]).any()
    assert (kind1 & cls["partner"] & ~cls["own"] & ~cls["past"]).any()
    for k in (kind1, kind2):                               # not only the first tile on either axis
        assert (k & (I >= TA)).any() and (k & (I >= 2 * TA)).any() and (k & (J >= TB)).any()
    # excluded rows contribute nothing to the statement: the recount's value is finite
    assert np.array_equal(bits(S["st"]["r"])[kind1], bits(S["st0"]["r"])[kind1])
    assert np.isfinite(S["st0"]["r"]).all() and (S["st0"]["r"][kind1] != 0.0).sum() >= 10
    nan2 = np.isnan(S["want2"])
    neg2 = np.signbit(S["want2"])
    assert (nan2 & neg2).sum() >= 3 and (nan2 & ~neg2).sum() >= 3
    other = ~kind1 & ~kind2
    assert other.sum() >= 10 and np.isfinite(S["st"]["r"][other]).all()


# --- CPU: the two forms against each other and against the reference ----------

def test_vector_form_equals_scalar_form():
    """Finite, ragged, with a constant sample: bit-equal, with and without the NaN rule."""
    vaf, dep, ns, st = geometry_set(40, 200, 5, 2)
    check_geometry_content(40, 200, 5, 2)
    want = scalar_matrix(vaf, dep, ns, 5, 2)
    assert np.array_equal(bits(matrix(st, 40)), bits(want))
    assert np.array_equal(bits(matrix(statement(vaf, dep, ns, 5, 2, x86=True), 40)), bits(want))


@pytest.mark.parametrize("min_depth", [2, 0])
def test_forms_agree_on_nonfinite_set(min_depth):
    """With the x86 NaN rule in both, the forms agree on every bit, NaN signs
    and payloads included; without it the vector form has the same finite cells."""
    S = nonfinite_set(min_depth)
    check_nonfinite_content(min_depth)
    n, _, min_snps = NF_SHAPE
    want = scalar_matrix(S["vaf"], S["dep"], S["ns"], min_snps, min_depth)
    got = matrix(statement(S["vaf"], S["dep"], S["ns"], min_snps, min_depth, x86=True), n)
    assert np.array_equal(bits(got), bits(want))
    plain = matrix(S["st"], n)
    assert np.array_equal(np.isnan(plain), np.isnan(want))
    assert np.array_equal(bits(plain)[~np.isnan(want)], bits(want)[~np.isnan(want)])


def load_fixture(path):
    """The rows the reference's sscanf keeps, for the well-formed fixture files."""
    x, d = [], []
    with open(path) as f:
        for line in f:
            if line.startswith("#") or line.startswith("CHR"):
                continue
            p = line.split()
            if len(p) != 9:
                continue
            try:
                int(p[1])
            except ValueError:
                continue
            x.append(parse_vaf(p[8]))
            d.append(int(p[7]))
    return x[:100000], d[:100000]


@pytest.mark.parametrize("name", ["nan_inf", "inf_both", "inf_pos", "const_eps", "ragged", "ragged_d0",
                                  "ragged_dneg"])
def test_forms_reproduce_golden_text(name):
    """The reference's recorded .corr text from both forms, "nan" / "-nan" included."""
    case = CASES[name]
    files, out, _, min_snps, min_depth = case_options(case["argv"])
    data = [load_fixture(os.path.join(CORR, fn)) for fn in files]
    names = []
    for fn in files:
        b = os.path.basename(fn)
        names.append(b[:b.index(".vaf")] if ".vaf" in b else b)
    ns = np.array([len(x) for x, _ in data], np.int32)
    vaf = np.zeros((len(data), int(ns.max())))
    dep = np.zeros(vaf.shape, np.int32)
    for s, (x, d) in enumerate(data):
        vaf[s, :len(x)], dep[s, :len(x)] = x, d
    fill_stride_area(vaf, dep, ns)
    n = len(ns)
    want = case["files"][out]
    assert corr_text(names, scalar_matrix(vaf, dep, ns, min_snps, min_depth)) == want
    assert corr_text(names, matrix(statement(vaf, dep, ns, min_snps, min_depth, x86=True), n)) == want
    plain = matrix(statement(vaf, dep, ns, min_snps, min_depth), n)
    if not np.isnan(plain).any():
        assert corr_text(names, plain) == want


@pytest.mark.parametrize("min_depth", [2, 0])
def test_nonfinite_set_matches_oracle(min_depth, tmp_path):
    S = nonfinite_set(min_depth)
    n, _, min_snps = NF_SHAPE
    paths, names = write_set(str(tmp_path), S["vaf"], S["dep"], S["ns"])
    text = oracle_text(str(tmp_path), paths, min_snps, min_depth)
    assert "\tnan" in text and "\t-nan" in text
    assert corr_text(names, scalar_matrix(S["vaf"], S["dep"], S["ns"], min_snps, min_depth)) == text
    assert corr_text(names, matrix(statement(S["vaf"], S["dep"], S["ns"], min_snps, min_depth, x86=True), n)) == text


def test_multi_tile_finite_set_matches_oracle(tmp_path):
    n, R, min_snps, min_depth = GEOMETRY[4]
    vaf, dep, ns, st = geometry_set(n, R, min_snps, min_depth)
    paths, names = write_set(str(tmp_path), vaf, dep, ns)
    assert corr_text(names, matrix(st, n)) == oracle_text(str(tmp_path), paths, min_snps, min_depth)


@pytest.mark.parametrize("n,R,min_snps,min_depth", GEOMETRY)
def test_geometry_sets_hold_their_content(n, R, min_snps, min_depth):
    check_geometry_content(n, R, min_snps, min_depth)


def test_raw_rejects_bad_row_counts():
    """n_snps[i] > stride and n_snps[i] < 0: VC_EINVAL, before anything is read."""
    import vafc
    vaf, dep = np.zeros((3, 8)), np.ones((3, 8), np.int32)
    corr = np.zeros((3, 3))
    for bad in ([8, 9, 8], [8, 8, -1]):
        ns = np.array(bad, np.int32)
        rc = vafc.lib().vc_corr_matrix_raw(vafc._ptr(vaf), vafc._ptr(dep), vafc._ptr(ns), 3, 8, 0, 0, vafc._ptr(corr),
                                           0, None)
        assert rc == vafc.VC_EINVAL


# --- GPU ---------------------------------------------------------------------

def assert_matrix_shape(got, n):
    assert got.shape == (n, n)
    assert (bits(np.diag(got)) == bits(np.ones(n))).all()
    assert np.array_equal(bits(got), bits(got.T))


@pytest.mark.gpu
@pytest.mark.parametrize("n,R,min_snps,min_depth", GEOMETRY)
def test_kernel_bit_exact_over_geometry(n, R, min_snps, min_depth):
    import vafc
    check_geometry_content(n, R, min_snps, min_depth)
    vaf, dep, ns, st = geometry_set(n, R, min_snps, min_depth)
    got, _ = vafc.correlation_matrix_raw(vaf, dep, ns, min_snps=min_snps, min_depth=min_depth)
    assert_matrix_shape(got, n)
    want = matrix(st, n)
    diff = np.argwhere(bits(got) != bits(want))
    assert len(diff) == 0, (len(diff), [(i, j, got[i, j].hex(), want[i, j].hex()) for i, j in diff[:5].tolist()])


@pytest.mark.gpu
def test_sample_set_matches_raw():
    """VafSamples.add + calculate_correlation_matrix: the bits of the raw call."""
    import vafc
    n, R, min_snps, min_depth = GEOMETRY[3]
    vaf, dep, ns, st = geometry_set(n, R, min_snps, min_depth)
    raw, _ = vafc.correlation_matrix_raw(vaf, dep, ns, min_snps=min_snps, min_depth=min_depth)
    S = vafc.VafSamples()
    for s in range(n):
        S.add("k%03d" % s, vaf[s, :ns[s]], dep[s, :ns[s]])
    assert [S.n_snps(s) for s in range(n)] == ns.tolist()
    got, _ = S.calculate_correlation_matrix(min_snps, min_depth)
    S.close()
    assert np.array_equal(bits(got), bits(raw))
    assert np.array_equal(bits(got), bits(matrix(st, n)))


@pytest.mark.gpu
@pytest.mark.parametrize("min_depth", [2, 0])
def test_kernel_nonfinite_rows(min_depth):
    """Non-finite values in excluded rows only: the finite value of the set with
    them zeroed (the recount).  In a valid row: the scalar statement's NaN-ness
    and sign.  Every other pair: the vector statement."""
    import vafc
    check_nonfinite_content(min_depth)
    S = nonfinite_set(min_depth)
    n, _, min_snps = NF_SHAPE
    got, _ = vafc.correlation_matrix_raw(S["vaf"], S["dep"], S["ns"], min_snps=min_snps, min_depth=min_depth)
    assert_matrix_shape(got, n)
    I, J, kind1, kind2 = S["st"]["I"], S["st"]["J"], S["kind1"], S["kind2"]
    g = got[I, J]
    assert np.isfinite(g[kind1]).all()
    assert np.array_equal(bits(g)[kind1], bits(S["st0"]["r"])[kind1])
    want2, g2 = S["want2"], g[kind2]
    assert np.array_equal(np.isnan(g2), np.isnan(want2))
    nan2 = np.isnan(want2)
    bad = np.flatnonzero(nan2 & (np.signbit(g2) != np.signbit(want2)))
    assert len(bad) == 0, [(int(I[kind2][k]), int(J[kind2][k])) for k in bad[:8]]
    assert np.array_equal(bits(g2)[~nan2], bits(want2)[~nan2])
    other = ~kind1 & ~kind2
    assert np.array_equal(bits(g)[other], bits(S["st"]["r"])[other])
