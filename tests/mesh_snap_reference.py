"""The statement of include/rnb_mesh_snap.h in numpy, written from the header: the network input of a position in float32, the rules of a round in float64 with every
operation rounded on its own, the final evaluation, the integer sums. The network is a callable, `evaluate(coords float32[n, 7]) -> float16[n, 16]`: the library's
forward_infer on the GPU, an analytic stand-in on the CPU. The device has to reproduce `expected_snap` bit for bit; nothing here calls the library."""
import numpy as np

MAX_ITERATIONS, MAX_IN_FLIGHT, RESIDUAL_LIMIT, Q_SCALE = 64, 1 << 22, 2.0 ** 8, 2.0 ** 24  # RNB_MESH_SNAP_*
UNSELECTED, CONVERGED, UNFINISHED, FLAT, LEASHED, OUTSIDE, STALLED, INVALID, REVERTED = range(9)
ACTIVE = 9  # never leaves a call
STATE_NAMES = ("unselected", "converged", "unfinished", "flat", "leashed", "outside", "stalled", "invalid", "reverted")
SNAP_STATS = ("n_selected",) + tuple("n_" + s for s in STATE_NAMES) + ("n_moved", "rounds", "max_displacement", "max_before", "max_after", "sum_before_q", "sum_after_q")
DEFAULTS = dict(iterations=3, level=0.0, tolerance=2.0 ** -13, max_step=1.0 / 128.0, max_displacement=1.0 / 64.0, min_gradient=0.25)


def network_input(v, aabb_min, aabb_diag):
    """float32[n, 7]: the clamped normalised position, 0, the warped direction from (0.5, 0.5, 0.5); float32 throughout, left to right."""
    v = np.asarray(v, np.float32).reshape(-1, 3)
    mn, diag, half, one = np.float32(aabb_min), np.float32(aabb_diag), np.float32(0.5), np.float32(1.0)
    with np.errstate(all="ignore"):
        d = v - half
        l = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
        c = np.zeros((len(v), 7), np.float32)
        c[:, 0:3] = np.fmin(np.fmax((v - mn) / diag, np.float32(0.0)), one)  # (fmax / fmin: a NaN becomes 0, as fmaxf makes it)
        c[:, 4:7] = (d / l[:, None] + one) * half
    assert c.dtype == np.float32
    return c


def _norm3(e):
    return np.sqrt((e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2])


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _q(r):
    a = np.abs(r)
    with np.errstate(invalid="ignore"):
        ok = a < RESIDUAL_LIMIT
    return np.where(ok, np.trunc(np.where(ok, a, 0.0) * Q_SCALE), 0.0).astype(np.uint64)


def attributes_of(out):
    """(colors float64[n, 3], normals float32[n, 3]) of half outputs: the logistic in float64 (the device's is float, with its own expf: close, not equal), the
    normals in float32 operation for operation: g / sqrt(g0 g0 + (g1 g1 + g2 g2)), zeros where the root is 0."""
    o = np.asarray(out, np.float16).astype(np.float32)
    with np.errstate(all="ignore"):
        colors = 1.0 / (1.0 + np.exp(-o[:, 0:3].astype(np.float64)))
        g = o[:, 4:7]
        gn = np.sqrt(g[:, 0] * g[:, 0] + (g[:, 1] * g[:, 1] + g[:, 2] * g[:, 2]))
        normals = np.where((gn > 0)[:, None], g / gn[:, None], np.float32(0.0)).astype(np.float32)
    return colors, normals


def expected_snap(verts, select, evaluate, aabb_min, aabb_diag, iterations=3, level=0.0, tolerance=2.0 ** -13, max_step=1.0 / 128.0, max_displacement=1.0 / 64.0,
                  min_gradient=0.25, attributes=(), colors=None, normals=None):
    """-> dict(verts, residual_before, residual_after, state, displacement, stats, out [the half outputs of the final evaluation, zeros for an unselected vertex],
    colors / normals when the input has them or they are asked for). The options are the floats of the struct, widened."""
    p0 = np.array(verts, np.float32).reshape(-1, 3)
    nv = len(p0)
    sel = np.ones(nv, bool) if select is None else (np.asarray(select).ravel() != 0)
    assert len(sel) == nv and 0 <= int(iterations) <= MAX_ITERATIONS
    level, tol, max_step, max_disp = (float(np.float32(x)) for x in (level, tolerance, max_step, max_displacement))
    mg2 = float(np.float32(min_gradient)) * float(np.float32(min_gradient))
    mn32, diag32 = np.float32(aabb_min), np.float32(aabb_diag)
    diag = float(diag32)
    p, prev = p0.copy(), p0.copy()
    a_prev = np.full(nv, np.inf)
    state = np.where(sel, ACTIVE, UNSELECTED).astype(np.uint32)
    r_before = np.zeros(nv)
    rounds = 0
    for k in range(1, int(iterations) + 2):
        act = np.flatnonzero(state == ACTIVE)
        if not len(act):
            break
        rounds += 1
        o = np.asarray(evaluate(network_input(p[act], mn32, diag32)), np.float16).astype(np.float64)
        with np.errstate(all="ignore"):
            r = o[:, 3] - level
            ar = np.abs(r)
            g = o[:, 4:7]
            if k == 1:
                r_before[act] = r
            finite = (ar < RESIDUAL_LIMIT) & np.isfinite(g).all(1)  # (a NaN compares false)
            gg = (g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2]
            t = r / gg
            d = (t[:, None] * g) * diag
            L = _norm3(d)
            long_ = L > max_step
            d = np.where(long_[:, None], d * (max_step / L)[:, None], d)
            Q = (p[act].astype(np.float64) - d).astype(np.float32)
            M = _norm3(Q.astype(np.float64) - p0[act].astype(np.float64))
            nq = (Q - mn32) / diag32
            outside = ((nq < 0) | (nq > 1)).any(1)
            same = (_bits(Q) == _bits(p[act])).all(1)
            st = np.full(len(act), ACTIVE, np.uint32)
            for cond, code in ((~finite, INVALID), (ar > a_prev[act], REVERTED), (ar <= tol, CONVERGED), (np.full(len(act), k == iterations + 1), UNFINISHED), (gg < mg2, FLAT),
                               (M > max_disp, LEASHED), (outside, OUTSIDE), (same, STALLED)):
                st = np.where((st == ACTIVE) & cond, code, st)  # the first rule that applies decides
        back = (st == INVALID) | (st == REVERTED)
        go = st == ACTIVE
        p[act[back]] = prev[act[back]]
        prev[act[go]] = p[act[go]]
        a_prev[act[go]] = ar[go]
        p[act[go]] = Q[go]
        state[act] = st
    assert not (state == ACTIVE).any()
    s = np.flatnonzero(sel)
    out = np.zeros((nv, 16), np.float16)
    if len(s):
        out[s] = np.asarray(evaluate(network_input(p[s], mn32, diag32)), np.float16)
    with np.errstate(all="ignore"):
        r_after = np.where(sel, out[:, 3].astype(np.float64) - level, 0.0)
        disp = np.where(sel, _norm3(p.astype(np.float64) - p0.astype(np.float64)).astype(np.float32), np.float32(0.0)).astype(np.float32)
    valid = sel & (state != INVALID)
    res = dict(verts=p, residual_before=r_before.astype(np.float32), residual_after=r_after.astype(np.float32), state=state, displacement=disp, out=out)
    want = set(attributes)
    assert want <= {"colors", "normals"}
    fresh = dict(zip(("colors", "normals"), attributes_of(out)))
    for name, given in (("colors", colors), ("normals", normals)):
        if given is None and name not in want:
            continue
        a = np.zeros((nv, 3), np.float64 if name == "colors" and name in want else np.float32) if given is None else np.array(given, np.float32).reshape(-1, 3).astype(
            np.float64 if name == "colors" and name in want else np.float32)
        if name in want:
            a[s] = fresh[name][s]
        res[name] = a
    stats = {"n_" + n: int((state == c).sum()) for c, n in enumerate(STATE_NAMES)}
    stats.update(n_selected=int(sel.sum()), n_moved=int((_bits(p) != _bits(p0)).any(1).sum()), rounds=rounds, max_displacement=float(disp.max()) if nv else 0.0,
                 max_before=float(np.abs(r_before[valid]).max()) if valid.any() else 0.0, max_after=float(np.abs(r_after[valid]).max()) if valid.any() else 0.0,
                 sum_before_q=int(_q(r_before[valid]).sum(dtype=np.uint64)), sum_after_q=int(_q(r_after[valid]).sum(dtype=np.uint64)))
    res["stats"] = stats
    return res
