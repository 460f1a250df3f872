"""GPU parity of the elementwise half of the prover, kernel by kernel (halo_amd/csrc/evals.hip): the seven Evals ops,
the division by X^n - 1, the three-kernel running product, the three fused gate-constraint passes and the geometric
combination, each called directly on both fields and compared word for word with the big-integer reference
tests/evals_ref.py.  No tolerances: every comparison is np.array_equal on the ark words.

Shapes are the smallest that reach each branch (lengths around the 256-thread and 2048-element blocks, a block count
above 256 for the scan's totals, `len - n` on either side of n for the division, a shifted witness that wraps from the
last block into the first); values come from EDGE (0, 1, p - 1, the top of the word range, every 29-bit limb and 64-bit
word boundary) and from draws over the whole of [0, p).  Every output buffer carries one guard row beyond its end: a
write one element past n fails an assertion.  The argument refusals of the same calls are in tests/test_evals_abi.py.
"""
import ctypes
import random

import numpy as np
import pytest

import evals_ref as E
import pasta as P

pytestmark = pytest.mark.gpu

FIELDS = E.FIELDS
SENTINEL = 0x5A5AA5A5C3C33C3C
SCAN_BLOCK = 2048


# ---------------------------------------------------------------------------------------------
# device buffers
# ---------------------------------------------------------------------------------------------
def dev(words, guard=False):
    """ark words (integers or an (n, 4) uint64 array) as a device tensor, optionally with a guard row behind them"""
    import torch

    a = words if isinstance(words, np.ndarray) else E.to_array(words)
    a = np.ascontiguousarray(a, dtype=np.uint64).reshape(-1, 4)
    if guard:
        a = np.concatenate([a, np.full((1, 4), SENTINEL, dtype=np.uint64)])
    return torch.from_numpy(a.view(np.int64)).cuda()


def out_buf(n):
    import torch

    return torch.full((n + 1, 4), SENTINEL, dtype=torch.int64, device="cuda")


def read(t, n):
    """the n elements of a guarded buffer, after asserting that its guard row is as it was"""
    import torch

    torch.cuda.synchronize()
    h = t.cpu().numpy().view(np.uint64)
    assert h.shape[0] == n + 1 and (h[n] == np.uint64(SENTINEL)).all(), "the guard row past the end was written"
    return h[:n]


def vp(t, row=0):
    return ctypes.c_void_p(t.data_ptr() + 32 * row) if t is not None else None


def stream():
    import torch

    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def same(got, exp, what=""):
    """got (array) == exp (ark words as integers or an array), naming the first differing element"""
    exp = exp if isinstance(exp, np.ndarray) else E.to_array(exp)
    assert got.shape == exp.shape, (what, got.shape, exp.shape)
    if not np.array_equal(got, exp):
        bad = np.nonzero((got != exp).any(axis=1))[0]
        raise AssertionError(f"{what}: {len(bad)} of {len(exp)} elements differ, the first at {bad[0]}: "
                             f"{E.from_array(got[bad[0]:bad[0] + 1])[0]:#x} for {E.from_array(exp[bad[0]:bad[0] + 1])[0]:#x}")


def fe1(W):
    return np.ascontiguousarray(E.to_array([W]))


def numpy_words(rng, n):
    """(n, 4) uint64 ark words uniform below 2^254 (every word of [0, p) but its last 2^126), built without a Python
    integer per element"""
    a = rng.integers(0, 2**64, size=(n, 4), dtype=np.uint64)
    a[:, 3] >>= np.uint64(2)
    return a


# ---------------------------------------------------------------------------------------------
# halo_evals_op_dev / halo_evals_op
# ---------------------------------------------------------------------------------------------
OP_NAMES = ["add", "sub", "mul", "scale", "add_scalar", "sub_scalar", "pow"]


def op_reference(op, a, b, s, e, m):
    """the reference on ark words: words -> values -> evals_ref.evals_op -> words"""
    return E.ark(E.evals_op(op, E.unark(a, m), E.unark(b, m) if b is not None else None,
                            E.unark([s], m)[0] if s is not None else None, e, m), m)


def run_op_dev(hal, fid, op, a, b, s, e, alias=None):
    """one halo_evals_op_dev launch; alias 'a' / 'b' makes the output that operand's own buffer"""
    n = len(a)
    ta, tb = dev(a, guard=True), (dev(b, guard=True) if b is not None else None)
    out = {None: out_buf(n), "a": ta, "b": tb}[alias]
    sc = fe1(s) if s is not None else None
    hal.check(hal.load().halo_evals_op_dev(fid, op, vp(ta), vp(tb), hal.ptr(sc), e, vp(out), n, stream()))
    got = read(out, n)
    for t, w, name in ((ta, a, "a"), (tb, b, "b")):  # an operand that is not the output is read only
        if t is not None and name != alias:
            same(read(t, n), w, f"{OP_NAMES[op]}: operand {name} after the call")
    return got


@pytest.mark.parametrize("tag,fid", FIELDS)
@pytest.mark.parametrize("n", [1, 255, 256, 257, 1000])
def test_evals_op_lengths(hal, tag, fid, n):
    """All seven ops at lengths around the 256-thread block (the `i >= n` guard decides at 1, 255, 257 and 1000), the
    binary ones also with the output aliasing either operand."""
    m = P.FIELDS[tag]
    rng = random.Random(n + fid)
    pool = E.EDGE(m) + E.full_range(rng, 1000, m)
    a, b = rng.sample(pool, n), rng.sample(pool, n)
    s = rng.randrange(m)
    for op in range(7):
        bb = b if op <= E.EV_MUL else None
        ss = s if E.EV_SCALE <= op <= E.EV_SUB_SCALAR else None
        exp = op_reference(op, a, bb, ss, 7, m)
        for alias in ((None, "a", "b") if op <= E.EV_MUL else (None, "a")):
            same(run_op_dev(hal, fid, op, a, bb, ss, 7, alias), exp, f"{OP_NAMES[op]} n={n} out={alias or 'own'}")


@pytest.mark.parametrize("tag,fid", FIELDS)
def test_evals_binary_edge_cross_product(hal, tag, fid):
    """add / sub / mul over EDGE x EDGE in one launch each: every pair of 0, 1, p - 1, 2^254, the limb and word
    boundaries, one and minus one (the borrow chain of fe_canon decides at p - 1 + 1, 0 - 1, (p - 1) + (p - 1))."""
    m = P.FIELDS[tag]
    edge = E.EDGE(m)
    a = [x for x in edge for _ in edge]
    b = [y for _ in edge for y in edge]
    for op in (E.EV_ADD, E.EV_SUB, E.EV_MUL):
        exp = op_reference(op, a, b, None, 0, m)
        for alias in (None, "a", "b"):
            same(run_op_dev(hal, fid, op, a, b, None, 0, alias), exp, f"{OP_NAMES[op]} EDGE x EDGE out={alias or 'own'}")


@pytest.mark.parametrize("tag,fid", FIELDS)
def test_evals_scalar_ops_edge_scalars(hal, tag, fid):
    """scale / add_scalar / sub_scalar with every EDGE word as the scalar (packed into limbs on the host), over EDGE
    and full-range elements."""
    m = P.FIELDS[tag]
    rng = random.Random(11 + fid)
    edge = E.EDGE(m)
    a = edge + E.full_range(rng, 30, m)
    for s in edge:
        for op in (E.EV_SCALE, E.EV_ADD_SCALAR, E.EV_SUB_SCALAR):
            same(run_op_dev(hal, fid, op, a, None, s, 0), op_reference(op, a, None, s, 0, m), f"{OP_NAMES[op]} s={s:#x}")


@pytest.mark.parametrize("tag,fid", FIELDS)
@pytest.mark.parametrize("e", [0, 1, 2, 7, 0x55555555, 0x80000000, 0xFFFFFFFF])
def test_evals_pow_exponents(hal, tag, fid, e):
    """x^e for exponents with the top bit, every other bit and all 32 bits set; 0^0 = 1."""
    m = P.FIELDS[tag]
    rng = random.Random(e % 1000 + fid)
    a = E.EDGE(m) + E.full_range(rng, 30, m)
    exp = op_reference(E.EV_POW, a, None, None, e, m)
    if e == 0:
        assert set(exp) == {P.R_MONT % m}
    same(run_op_dev(hal, fid, E.EV_POW, a, None, None, e), exp, f"pow e={e:#x}")


@pytest.mark.parametrize("tag,fid", FIELDS)
def test_evals_op_host_form_ragged(hal, tag, fid):
    """halo_evals_op (host arrays, staged through the scratch) at a length that is no multiple of the block."""
    m = P.FIELDS[tag]
    n = 257
    rng = random.Random(21 + fid)
    pool = E.EDGE(m) + E.full_range(rng, 300, m)
    a, b = rng.sample(pool, n), rng.sample(pool, n)
    s = rng.choice(E.EDGE(m))
    A, B = np.ascontiguousarray(E.to_array(a)), np.ascontiguousarray(E.to_array(b))
    for op in range(7):
        out = np.full((n + 1, 4), SENTINEL, dtype=np.uint64)
        hal.check(hal.load().halo_evals_op(fid, op, hal.ptr(A), hal.ptr(B) if op <= 2 else None,
                                           hal.ptr(fe1(s)) if 3 <= op <= 5 else None, 0x80000001, hal.ptr(out), n))
        assert (out[n] == np.uint64(SENTINEL)).all(), "the guard row past the end was written"
        same(out[:n], op_reference(op, a, b if op <= 2 else None, s if 3 <= op <= 5 else None, 0x80000001, m),
             f"host {OP_NAMES[op]}")
    same(A, a, "host operand a")
    same(B, b, "host operand b")


# ---------------------------------------------------------------------------------------------
# halo_divide_by_vanishing_dev
# ---------------------------------------------------------------------------------------------
DIV_SHAPES = [(1, 1), (2, 1), (7, 1), (5, 5), (6, 5), (64, 64), (65, 64), (127, 64), (128, 64), (129, 64), (505, 64),
              (300, 3), (600, 512)]


@pytest.mark.parametrize("tag,fid", FIELDS)
@pytest.mark.parametrize("ln,n", DIV_SHAPES)
def test_divide_by_vanishing_shapes(hal, tag, fid, ln, n):
    """Every quotient and remainder entry: one term per lane up to a hundred ((300, 3): len - n > n, two blocks of
    quotient lanes; (600, 512): n > len - n, two blocks of remainder lanes), no quotient at all when len == n."""
    m = P.FIELDS[tag]
    rng = random.Random(ln * 1000 + n + fid)
    c = E.full_range(rng, ln, m)
    for i in rng.sample(range(ln), ln // 3 + 1):
        c[i] = rng.choice(E.EDGE(m))
    qv, rv = E.div_vanishing(E.unark(c, m), n, m)
    tc = dev(c, guard=True)
    q = out_buf(ln - n) if ln > n else None
    r = out_buf(n)
    hal.check(hal.load().halo_divide_by_vanishing_dev(fid, vp(tc), ln, n, vp(q), vp(r), stream()))
    same(read(r, n), E.ark(rv, m), f"remainder ({ln}, {n})")
    if q is not None:
        same(read(q, ln - n), E.ark(qv, m), f"quotient ({ln}, {n})")
    same(read(tc, ln), c, "the coefficients after the call")


# ---------------------------------------------------------------------------------------------
# halo_evals_scan_dev
# ---------------------------------------------------------------------------------------------
def run_scan(hal, fid, reverse, words, n, st=None):
    tin, out = dev(words, guard=True), out_buf(n)
    hal.check(hal.load().halo_evals_scan_dev(fid, reverse, vp(tin), vp(out), n, st or stream()))
    return tin, out


def zeroed(exp, j, reverse):
    """the running product of an input whose element j is zero, from that of the same input without the zero:
    everything on the far side of j is zero, the near side untouched"""
    z = exp.copy()
    if reverse:
        z[:j + 1] = 0
    else:
        z[j:] = 0
    return z


@pytest.mark.parametrize("tag,fid", FIELDS)
@pytest.mark.parametrize("reverse", [0, 1])
@pytest.mark.parametrize("n", [1, 2, 7, 8, 9, 2047, 2048, 2049, 4099])
def test_scan_small_lengths(hal, tag, fid, reverse, n):
    """Prefix and suffix products at lengths around a thread's 8 elements and a block's 2048, every position, against
    the sequential product: full-range words, all ones, all minus one (the result alternates), and one zero at each
    of the block's corners."""
    m = P.FIELDS[tag]
    rng = random.Random(n * 2 + reverse + 100 * fid)
    base = E.full_range(rng, n, m)
    for i in rng.sample(range(n), n // 8 + 1):
        base[i] = rng.choice([W for W in E.EDGE(m) if W])
    one, minus_one = P.R_MONT % m, m - P.R_MONT % m
    families = {"random": base, "ones": [one] * n, "minus one": [minus_one] * n}
    for j in sorted({0, 5, 2047, 2048, n - 1}):
        if j < n:
            families[f"zero at {j}"] = base[:j] + [0] + base[j + 1:]
    exp_random = None
    for name, words in families.items():
        exp = E.to_array(E.ark(E.scan(E.unark(words, m), reverse, m), m))
        tin, out = run_scan(hal, fid, reverse, words, n)
        same(read(out, n), exp, f"scan n={n} reverse={reverse} {name}")
        same(read(tin, n), words, "the input after the call")
        if name == "random":
            exp_random = exp
        elif name == "minus one":
            signs = [(n - i) % 2 if reverse else (i + 1) % 2 for i in range(n)]
            assert E.from_array(exp) == [minus_one if s else one for s in signs]
        elif name.startswith("zero"):
            assert np.array_equal(exp, zeroed(exp_random, int(name.split()[-1]), reverse))


@pytest.fixture(scope="module")
def big_scan_reference():
    """The input of the 258-block scan and its running products, made once per (field, direction) and left unchanged."""
    cache = {}

    def get(tag, reverse):
        m = P.FIELDS[tag]
        n = 257 * SCAN_BLOCK + 5
        if tag not in cache:
            rng = np.random.default_rng({"fp": 258, "fq": 259}[tag])
            a = numpy_words(rng, n)
            edge = [W for W in E.EDGE(m) if W]
            for k, i in enumerate(rng.choice(n, size=4 * len(edge), replace=False)):
                a[i] = E.to_array([edge[k % len(edge)]])[0]
            a.setflags(write=False)
            cache[tag] = {"in": a, "ints": E.from_array(a)}
        c = cache[tag]
        if reverse not in c:
            c[reverse] = E.to_array(E.scan_words(c["ints"], reverse, m))
            c[reverse].setflags(write=False)
        return n, c["in"], c[reverse]

    return get


@pytest.mark.parametrize("tag,fid", FIELDS)
@pytest.mark.parametrize("reverse", [0, 1])
def test_scan_258_blocks(hal, big_scan_reference, tag, fid, reverse):
    """n = 257 * 2048 + 5: 258 block totals, so k_scan_totals gives each of its first 129 threads two totals and leaves
    the rest idle, and the last block holds five elements.  Every position, against the sequential product kept in the
    Montgomery domain; then all ones, all minus one, and a zero at each corner."""
    m = P.FIELDS[tag]
    n, words, exp = big_scan_reference(tag, reverse)
    tin, out = run_scan(hal, fid, reverse, words, n)
    same(read(out, n), exp, f"scan n={n} reverse={reverse} random")
    same(read(tin, n), words, "the input after the call")
    one, minus_one = P.R_MONT % m, m - P.R_MONT % m
    for name, W in (("ones", one), ("minus one", minus_one)):
        const = np.repeat(E.to_array([W]), n, axis=0)
        exp_c = E.to_array(E.scan_words([W] * n, reverse, m))
        if W == minus_one:  # out[i] is minus one to the number of factors
            neg = (np.arange(n)[::-1] if reverse else np.arange(n)) % 2 == 0
            assert np.array_equal(exp_c, np.where(neg[:, None], E.to_array([minus_one]), E.to_array([one])))
        _, out = run_scan(hal, fid, reverse, const, n)
        same(read(out, n), exp_c, f"scan n={n} reverse={reverse} {name}")
    for j in (0, 5, 2047, 2048, n - 1):
        w0 = words.copy()
        w0[j] = 0
        _, out = run_scan(hal, fid, reverse, w0, n)
        same(read(out, n), zeroed(exp, j, reverse), f"scan n={n} reverse={reverse} zero at {j}")


# ---------------------------------------------------------------------------------------------
# halo_gate_constraints_dev
# ---------------------------------------------------------------------------------------------
GATE_SHAPES = [(1, 0), (8, 1), (8, 8), (256, 8), (512, 8), (512, 1), (512, 511)]
GATE_GROUPS = ["q0 w0", "q1 w1", "q2 w2", "q3 w0 w1", "q4 constant", "q5 poseidon", "q6 affine add", "q7 affine mul",
               "q8 eq", "q9 range check"]


def run_gate(hal, fid, w, r, q, pi, mds9, N, shift, st=None):
    """one halo_gate_constraints_dev call on ark words: w (16), r (15), q (10) vectors of N, pi, the 9 MDS words"""
    vecs = np.concatenate([c if isinstance(c, np.ndarray) else E.to_array(c) for c in list(w) + list(r) + list(q) + [pi]])
    t = dev(vecs, guard=True)
    ptr = lambda lo, k: (ctypes.c_void_p * k)(*[t.data_ptr() + 32 * N * (lo + i) for i in range(k)])
    out = out_buf(N)
    m9 = np.ascontiguousarray(E.to_array(mds9))
    hal.check(hal.load().halo_gate_constraints_dev(fid, ptr(0, 16), ptr(16, 15), ptr(31, 10), vp(t, 41 * N), hal.ptr(m9), N,
                                                   shift, vp(out), st or stream()))
    return t, vecs, out


def gate_reference(w, r, q, pi, mds9, shift, m):
    u = lambda vs: [E.unark(c, m) for c in vs]
    mv = E.unark(mds9, m)
    return E.ark(E.gate_constraints(u(w), u(r), u(q), E.unark(pi, m), [mv[0:3], mv[3:6], mv[6:9]], shift, m), m)


def check_gate(hal, fid, w, r, q, pi, mds9, N, shift, m, what):
    t, vecs, out = run_gate(hal, fid, w, r, q, pi, mds9, N, shift)
    exp = gate_reference(w, r, q, pi, mds9, shift, m)
    same(read(out, N), exp, f"gate N={N} shift={shift} {what}")
    same(read(t, 42 * N), vecs, "the inputs after the call")
    return exp


def gate_random(rng, N, m):
    vec = lambda: E.full_range(rng, N, m)
    return ([vec() for _ in range(16)], [vec() for _ in range(15)], [vec() for _ in range(10)], vec(),
            E.full_range(rng, 9, m))


@pytest.mark.parametrize("tag,fid", FIELDS)
@pytest.mark.parametrize("N,shift", GATE_SHAPES)
def test_gate_constraints_values(hal, tag, fid, N, shift):
    """f_gc of every element against the `*_generic` forms on integers: full-range inputs, every word p - 1, only the
    constant selector and the public input, the zero-difference branches of both affine groups, and degenerate MDS
    rows.  N = 512 is two blocks: with shift 8, 1 and 511 the shifted witness of the last block is read from the first."""
    m = P.FIELDS[tag]
    rng = random.Random(N * 1000 + shift + fid)
    zero, top = [0] * N, [m - 1] * N
    w, r, q, pi, mds9 = gate_random(rng, N, m)
    check_gate(hal, fid, w, r, q, pi, mds9, N, shift, m, "full-range")
    check_gate(hal, fid, [top] * 16, [top] * 15, [top] * 10, top, [m - 1] * 9, N, shift, m, "every word p - 1")
    q4 = [zero] * 4 + [q[4]] + [zero] * 5
    exp = check_gate(hal, fid, [zero] * 16, [zero] * 15, q4, pi, [0] * 9, N, shift, m, "only q4 and pi")
    assert exp == [(a + b) % m for a, b in zip(q[4], pi)]
    # affine add reads (xp, yp, xq, yq) = w[0..4], affine mul (xg, yg, xq, yq) = w[3], w[4], w[6], w[7]: equal points,
    # then opposite ones, in both
    neg = lambda c: [(m - x) % m for x in c]
    wa = list(w)
    wa[2], wa[3] = wa[0], wa[1]
    wa[6], wa[7] = wa[3], wa[4]
    check_gate(hal, fid, wa, r, q, pi, mds9, N, shift, m, "equal points (zero differences)")
    wb = list(w)
    wb[2], wb[3] = wb[0], neg(wb[1])
    wb[6], wb[7] = wb[3], neg(wb[4])
    check_gate(hal, fid, wb, r, q, pi, mds9, N, shift, m, "opposite points (zero sums)")
    one = P.R_MONT % m
    for row, triple in enumerate(([0, 0, 0], [one, one, one], [m - one, one, 0])):  # the values (0,0,0), (1,1,1), (-1,1,0)
        md = list(mds9)
        md[3 * row:3 * row + 3] = triple
        check_gate(hal, fid, w, r, q, pi, md, N, shift, m, f"MDS row {row} = {E.unark(triple, m)}")
        md[3 * row:3 * row + 3] = [[0, 0, 0], [1, 1, 1], [m - 1, 1, 0]][row]  # and the same as raw words
        check_gate(hal, fid, w, r, q, pi, md, N, shift, m, f"MDS row {row} words {md[3 * row:3 * row + 3]}")


@pytest.mark.parametrize("tag,fid", FIELDS)
@pytest.mark.parametrize("N,shift", GATE_SHAPES)
@pytest.mark.parametrize("k", range(10), ids=[g.replace(" ", "_") for g in GATE_GROUPS])
def test_gate_constraints_selector_isolation(hal, tag, fid, N, shift, k):
    """One selector all ones, the other nine and the public input zero, over a full-range witness: f_gc is then one
    constraint group alone, and a failure names it."""
    m = P.FIELDS[tag]
    rng = random.Random(N * 1000 + shift + 50 + fid)
    w, r, _, _, mds9 = gate_random(rng, N, m)
    zero, ones = [0] * N, [P.R_MONT % m] * N
    q = [ones if j == k else zero for j in range(10)]
    check_gate(hal, fid, w, r, q, zero, mds9, N, shift, m, f"selector {k} alone ({GATE_GROUPS[k]})")


@pytest.mark.parametrize("tag,fid", FIELDS)
def test_gate_constraints_smaller_call_after_larger(hal, tag, fid):
    """N = 8 straight after N = 512: the partial vectors live in a buffer that only grows, and the second call's second
    vector starts inside the first call's first."""
    m = P.FIELDS[tag]
    rng = random.Random(77 + fid)
    big, small = gate_random(rng, 512, m), gate_random(rng, 8, m)
    t1, _, out1 = run_gate(hal, fid, *big, 512, 8)
    t2, _, out2 = run_gate(hal, fid, *small, 8, 1)  # queued behind the first without a synchronisation
    same(read(out2, 8), gate_reference(*small, 1, m), "gate N=8 after N=512")
    same(read(out1, 512), gate_reference(*big, 8, m), "gate N=512 before N=8")


# ---------------------------------------------------------------------------------------------
# halo_poly_lincomb_dev
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag,fid", FIELDS)
@pytest.mark.parametrize("k", [0, 1, 2, 43, 64])
def test_poly_lincomb_ragged(hal, tag, fid, k):
    """sum_i zeta^i p_i over k ragged inputs (length 0 as a null pointer), with the output as long as the longest
    input and 70 longer (the tail is written as zeros), at zeta = 0, 1, -1 and a full-range one."""
    m = P.FIELDS[tag]
    rng = random.Random(k + 100 * fid)
    edge = E.EDGE(m)
    choices = [0, 1, 255, 256, 257, 300]
    for draw in range(3 if k in (1, 2) else 1):
        lens = [rng.choice(choices) for _ in range(k)]
        if k >= 43:
            lens[0], lens[-1] = 300, 0  # the longest first, an absent one last (the Horner pass starts there)
        polys = [[rng.choice(edge) if rng.random() < 0.25 else rng.randrange(m) for _ in range(ln)] for ln in lens]
        ts = [dev(p, guard=True) if p else None for p in polys]
        ptrs = (ctypes.c_void_p * max(k, 1))(*[t.data_ptr() if t is not None else None for t in ts]) if k else None
        clens = (ctypes.c_size_t * max(k, 1))(*lens) if k else None
        vals = [E.unark(p, m) for p in polys]
        for zeta in (0, 1, m - 1, rng.randrange(m)):
            for n_out in (max(lens, default=0), max(lens, default=0) + 70):
                out = out_buf(n_out)
                hal.check(hal.load().halo_poly_lincomb_dev(fid, ptrs, clens, k, hal.ptr(fe1(P.to_mont(zeta, m))),
                                                           vp(out) if n_out else None, n_out, stream()))
                exp = E.ark(E.lincomb(vals, zeta, n_out, m), m)
                assert exp[max(lens, default=0):] == [0] * (n_out - max(lens, default=0))
                same(read(out, n_out), exp, f"lincomb k={k} lens={lens} zeta={zeta:#x} n_out={n_out}")
        for t, p in zip(ts, polys):
            if t is not None:
                same(read(t, len(p)), p, "an input after the calls")


# ---------------------------------------------------------------------------------------------
# two streams: the shared scan_tmp and gate_tmp
# ---------------------------------------------------------------------------------------------
def test_scan_and_gate_on_two_streams(hal):
    """Four rounds with a forward scan (n = 2^18 + 5) on one torch stream and a reverse scan plus a gate evaluation
    (N = 2^15) on another, nothing synchronised in between: the block totals and the gate's partial vectors are
    device-global buffers that every call fences for its stream (ScratchUse), so each result equals the same call made
    alone, and the scans equal the sequential product."""
    import torch

    tag, fid = "fp", 0
    m = P.FIELDS[tag]
    n, N, rounds = (1 << 18) + 5, 1 << 15, 4
    rng = np.random.default_rng(2024)
    fwd_in = [numpy_words(rng, n) for _ in range(rounds)]
    rev_in = [numpy_words(rng, n) for _ in range(rounds)]
    gate_in = numpy_words(rng, 42 * N)
    gw, gr, gq = ([gate_in[N * (lo + i):N * (lo + i + 1)] for i in range(k)] for lo, k in ((0, 16), (16, 15), (31, 10)))
    gpi, mds9 = gate_in[41 * N:], E.from_array(numpy_words(rng, 9))
    shifts = [8, 1, N - 1, 4097]
    # alone, on the current stream, each call synchronised before the next
    alone = []
    for k in range(rounds):
        row = []
        for call in (lambda: run_scan(hal, fid, 0, fwd_in[k], n)[1], lambda: run_scan(hal, fid, 1, rev_in[k], n)[1],
                     lambda: run_gate(hal, fid, gw, gr, gq, gpi, mds9, N, shifts[k])[2]):
            out = call()
            row.append(read(out, out.shape[0] - 1).copy())
        alone.append(row)
    for k in range(rounds):
        same(alone[k][0], E.scan_words(E.from_array(fwd_in[k]), 0, m), f"forward scan {k} alone")
        same(alone[k][1], E.scan_words(E.from_array(rev_in[k]), 1, m), f"reverse scan {k} alone")
    # together
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    p1, p2 = ctypes.c_void_p(s1.cuda_stream), ctypes.c_void_p(s2.cuda_stream)
    L = hal.load()
    tf = [dev(a, guard=True) for a in fwd_in]
    tr = [dev(a, guard=True) for a in rev_in]
    tg = dev(gate_in, guard=True)
    ptr = lambda lo, k: (ctypes.c_void_p * k)(*[tg.data_ptr() + 32 * N * (lo + i) for i in range(k)])
    dw, dr, dq = ptr(0, 16), ptr(16, 15), ptr(31, 10)
    m9 = np.ascontiguousarray(E.to_array(mds9))
    outs = [(out_buf(n), out_buf(n), out_buf(N)) for _ in range(rounds)]
    torch.cuda.synchronize()
    for k in range(rounds):
        hal.check(L.halo_evals_scan_dev(fid, 0, vp(tf[k]), vp(outs[k][0]), n, p1))
        hal.check(L.halo_evals_scan_dev(fid, 1, vp(tr[k]), vp(outs[k][1]), n, p2))
        hal.check(L.halo_gate_constraints_dev(fid, dw, dr, dq, vp(tg, 41 * N), hal.ptr(m9), N, shifts[k], vp(outs[k][2]), p2))
    torch.cuda.synchronize()
    for k in range(rounds):
        for j, (name, ln) in enumerate((("forward scan", n), ("reverse scan", n), ("gate", N))):
            same(read(outs[k][j], ln), alone[k][j], f"round {k}: {name} beside the other stream")
