"""A float64 reference of the per-step bodies of the reblurring pass -- the general 2-D stencil and the rank-1 body of
csrc/conv.hip, the workgroup form of the tile-spectrum body (csrc/conv_fft.hip) --, a restatement of the phase list
finish_record (csrc/estimate.hip) builds for the general body, and a float64 walk of that list the way the body walks it; in
plain NumPy.  A helper of tests/test_stencil_ref_cpu.py and tests/test_gpu_stencil_conformance.py: the case families both walk
are listed at the end (A: every tap position in every radius class; B: the structures of the phase list only sparse lists
reach; C: the rank-1 body; D: the tile-spectrum body; E: adaptive support; and the geometry edges).

The semantics are the ones include/polyblur_hip.h states for pb_set_kernels: under PB_ZERO the taps as given, applied as a
correlation with zero outside the Hp x Wp domain; under PB_WRAP the true circular convolution over the domain."""
import functools

import numpy as np

import window_ref as wr

PAD, KSIZE = wr.PAD, wr.KSIZE
WRAP, ZERO = 0, 1                                   # pb_boundary
FULL, ADAPTIVE, FORCE_GENERAL = 0, 1, 16            # pb_support
CLASSES = (4, 6, 8, 10, 12)                         # the radius classes of the general body
RANK1_CLASSES = (4, 8, 12)                          # the templates of the rank-1 body and the halo classes of the workgroup form
FILLER = (KSIZE * 32) << 16                         # the filler descriptor: LDS offset 0, the all-zero tap row 25
U32 = 2.0 ** -24                                    # fp32 unit roundoff


# ---------------------------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------------------------
def _extend(x, boundary, m, mutant=None):
    """(C, Hp, Wp) -> (C, Hp + 2 m, Wp + 2 m): the domain continued by m samples on every side under the boundary model.
    mutant 'clamp': the edge sample where zero is due; 'period': wrap with the period Wp - 1 along x."""
    Hp, Wp = x.shape[-2:]
    iy, ix = np.arange(-m, Hp + m), np.arange(-m, Wp + m)
    if boundary == WRAP:
        return x[..., (iy % Hp)[:, None], (ix % (Wp - 1 if mutant == "period" else Wp))[None, :]]
    if mutant == "clamp":
        return x[..., np.clip(iy, 0, Hp - 1)[:, None], np.clip(ix, 0, Wp - 1)[None, :]]
    out = np.zeros(x.shape[:-2] + (Hp + 2 * m, Wp + 2 * m))
    out[..., m:m + Hp, m:m + Wp] = x
    return out


def _apply(x, k, boundary, mutant=None):
    """one image (C, Hp, Wp) float64, one odd-sided kernel (kh, kw) float64 centred at (kh // 2, kw // 2) -> K x by direct
    shifted sums over the non-zero taps.  PB_ZERO: out[p] = sum k[d] x[p + d]; PB_WRAP: out[p] = sum k[d] x[p - d], indices
    modulo the domain.  mutant 'flip': the other of the two."""
    Hp, Wp = x.shape[-2:]
    cy, cx = k.shape[0] // 2, k.shape[1] // 2
    m = max(cy, cx)
    xe = _extend(x, boundary, m, mutant)
    conv = (boundary == WRAP) != (mutant == "flip")
    out = np.zeros(x.shape)
    for i, j in zip(*np.nonzero(k)):
        dy, dx = (cy - i, cx - j) if conv else (i - cy, j - cx)
        out += k[i, j] * xe[..., m + dy:m + dy + Hp, m + dx:m + dx + Wp]
    return out


def correlate64(xp, taps, boundary, mutant=None):
    """xp: (B, C, Hp, Wp); taps: (B, 25, 25) fp32 values taken exactly -> (K xp, S = |K| |xp|), both float64"""
    x = np.asarray(xp, np.float64)
    k = np.asarray(taps, np.float64)
    assert x.ndim == 4 and k.shape == (x.shape[0], KSIZE, KSIZE), (x.shape, k.shape)
    y = np.stack([_apply(x[b], k[b], boundary, mutant) for b in range(x.shape[0])])
    s = np.stack([_apply(np.abs(x[b]), np.abs(k[b]), boundary, mutant) for b in range(x.shape[0])])
    return y, s


def inverse_filter64(x, taps, alpha, beta, boundary):
    """x: (B, C, H, W) -> replicate pad by 12, the three Horner steps of deblurring.py:122-138 with K under the boundary, crop;
    float64, unclamped"""
    x = np.asarray(x, np.float64)
    k = np.asarray(taps, np.float64)
    xp = np.pad(x, [(0, 0), (0, 0), (PAD, PAD), (PAD, PAD)], mode="edge")
    a3, a2, a1, b = wr.coefficients(alpha, beta)
    K = lambda t: np.stack([_apply(t[i], k[i], boundary) for i in range(t.shape[0])])
    t = K(a3 * xp) + a2 * xp
    t = K(t) + a1 * xp
    y = K(t) + b * xp
    return y[..., PAD:-PAD, PAD:-PAD]


# ---------------------------------------------------------------------------------------------
# the phase list of the general body (csrc/estimate.hip: finish_record)
# ---------------------------------------------------------------------------------------------
def marginals(taps):
    """-> (kx, ky) symmetrised, as the record holds them (float64 sums of the fp32 taps)"""
    k = np.asarray(taps, np.float64)
    kx, ky = k.sum(axis=0), k.sum(axis=1)
    return 0.5 * (kx + kx[::-1]), 0.5 * (ky + ky[::-1])


def residual(taps):
    """sum |k - ky (x) kx| with the symmetrised marginals: the record is rank-1 where this is < 1e-6"""
    kx, ky = marginals(taps)
    return float(np.abs(np.asarray(taps, np.float64) - np.outer(ky, kx)).sum())


def descriptor(R, row, q):
    """byte offset of chunk q of window row `row` in the (64 + 2 R)-wide staged tile | index of its first tap in gtaps << 16"""
    off = PAD - R
    return ((row * (64 + 2 * R) + 4 * q) * 4) | (((row + off) * 32 + 4 * q + off) << 16)


def phase_list(taps, support):
    """-> (separable, radius, nphase[3], [(kind, row, q)]) of one 25 x 25 fp32 tap set: the list in the order the body walks
    it, fillers as (kind, None, None).  radius: from the live rows and columns -- not exactly 0.0f (FULL), a symmetrised
    marginal >= 1e-8 (ADAPTIVE) --, rounded up to 4, 6, 8, 10 or 12.  Chunk q of window row `row` (kernel row row + 12 - R) sees
    the taps k[row + 12 - R][4 q + 12 - R - 3 .. + 3] and is live if one of them is non-zero (FULL) or >= 1e-10 (ADAPTIVE)."""
    k32 = np.asarray(taps, np.float32)
    assert k32.shape == (KSIZE, KSIZE)
    k = k32.astype(np.float64)
    adaptive = (support & 15) == ADAPTIVE
    kx, ky = marginals(k32)
    sep = int(residual(k32) < 1e-6 and not (support & FORCE_GENERAL))
    if adaptive:
        live = (np.abs(kx) >= 1e-8) | (np.abs(ky) >= 1e-8)
    else:
        live = (k != 0).any(axis=0) | (k != 0).any(axis=1)
    rad = 0
    if live.any():
        idx = np.nonzero(live)[0]
        rad = max(PAD - idx[0], idx[-1] - PAD)
    R = next(c for c in CLASSES if rad <= c)
    off, nq = PAD - R, R // 2 + 1
    groups = ([], [], [])
    for row in range(2 * R + 1):
        for q in range(nq):
            js = [j for j in range(4 * q + off - 3, 4 * q + off + 4) if 0 <= j < KSIZE]
            t = np.abs(k32[row + off, js])
            if (t >= np.float32(1e-10)).any() if adaptive else (t != 0).any():
                groups[1 if q == 0 else (2 if q == nq - 1 else 0)].append((row, q))
    phases, nphase = [], []
    for kind in range(3):
        phases += [(kind, row, q) for row, q in groups[kind]]
        if len(groups[kind]) & 1:
            phases.append((kind, None, None))
        nphase.append(len(groups[kind]) + (len(groups[kind]) & 1))
    return sep, R, nphase, phases


def descriptors(R, phases):
    return [FILLER if row is None else descriptor(R, row, q) for _, row, q in phases]


def support_margin(taps):
    """how far the adaptive policy's thresholds are from deciding otherwise in fp32: the smallest ratio (>= 1) between a symmetrised
    marginal and 1e-8"""
    kx, ky = marginals(taps)
    m = np.concatenate([np.abs(kx), np.abs(ky)])
    m = m[m > 0]
    return float(np.min(np.maximum(m / 1e-8, 1e-8 / m)))


# ---------------------------------------------------------------------------------------------
# the walk: what the listed phases evaluate
# ---------------------------------------------------------------------------------------------
_EW = 4                                             # columns the effective kernels keep on either side of the 25


def effective_taps(taps, R, phases, mutant=None):
    """-> (4, 25, 33) float64: per output column modulo 4 (o, counted from the left edge of the output region), the kernel the
    walk of the list applies; column index j + 4 for the tap column j.  A thread holds outputs o = 0 .. 3; in the phase
    (row, q) window element e = 0 .. 3 of the chunk feeds output o with the tap k[row + 12 - R][4 q + 12 - R + e - o] (two packed
    FMAs per element: conv.hip, chunk_fma2); kind 1 leaves out (e < 2, o >= 2), kind 2 (e >= 2, o < 2) -- taps outside the box.
    A filler reads the all-zero tap row against window row 0, chunk 0.
    mutants: ('drop', kind) the last live phase of that kind's group is not evaluated; 'filler' a filler is evaluated with the
    previous phase's taps; 'swap' the two taps of every odd-aligned pair (the pairs odd elements read) are exchanged."""
    k = np.asarray(taps, np.float64)
    off = PAD - R
    eff = np.zeros((4, KSIZE, KSIZE + 2 * _EW))
    tap = lambda r, j: k[r, j] if 0 <= j < KSIZE else 0.0
    if mutant is not None and mutant[0] == "drop":
        last = max(i for i, (kind, row, _) in enumerate(phases) if kind == mutant[1] and row is not None)
        phases = phases[:last] + phases[last + 1:]
    prev = None
    for kind, row, q in phases:
        if row is None:
            if mutant != "filler" or prev is None:
                continue
            trow, tq, wrow, wq = prev[0] + off, prev[1], 0, 0
        else:
            trow, tq, wrow, wq = row + off, q, row, q
            prev = (row, q)
        for e in range(4):
            for o in range(4):
                if (kind == 1 and e < 2 and o >= 2) or (kind == 2 and e >= 2 and o < 2):
                    continue
                oo = o ^ 1 if (mutant == "swap" and e & 1) else o
                eff[o, wrow + off, 4 * wq + off + e - o + _EW] += tap(trow, 4 * tq + off + e - oo)
    return eff


def walk64(xp, taps, phases, boundary, mutant=None, radii=None):
    """the stencil as the body evaluates it, phase by phase in float64: only the seven taps of each listed chunk against its four
    window elements.  phases: one list per image (phase_list's fourth value), radii: their classes (default: phase_list's under
    FULL | FORCE_GENERAL).  mutant: None; effective_taps' ('drop', kind), 'filler', 'swap'; 'clamp', 'period', 'flip' (_apply)."""
    x = np.asarray(xp, np.float64)
    out = np.zeros(x.shape)
    for b in range(x.shape[0]):
        R = radii[b] if radii is not None else phase_list(taps[b], FULL | FORCE_GENERAL)[1]
        lm = mutant if mutant in ("filler", "swap") or (mutant is not None and mutant[0] == "drop") else None
        eff = effective_taps(taps[b], R, phases[b], lm)
        bm = mutant if lm is None else None
        if (eff == eff[0]).all():
            out[b] = _apply(x[b], eff[0], boundary, bm)
        else:
            for o in range(4):
                out[b][..., o::4] = _apply(x[b], eff[o], boundary, bm)[..., o::4]
    return out


def walked_taps_equal(taps, R, phases):
    """the walk applies every tap exactly once to every output: all four effective kernels are the taps themselves"""
    eff = effective_taps(taps, R, phases)
    want = np.zeros(eff.shape[1:])
    want[:, _EW:_EW + KSIZE] = np.asarray(taps, np.float64)
    return all(np.array_equal(eff[o], want) for o in range(4))


def dropped_mass(taps, R, phases):
    """the largest |tap| mass the walk leaves out for any output column (ADAPTIVE: rows / columns outside the box, dead chunks)"""
    eff = effective_taps(taps, R, phases)
    want = np.zeros(eff.shape[1:])
    want[:, _EW:_EW + KSIZE] = np.asarray(taps, np.float64)
    return float(max(np.abs(eff[o] - want).sum() for o in range(4)))


def rank1_64(xp, kx, ky, R, boundary, mutant=None):
    """the rank-1 body in float64: symmetrised marginals, taps 0 .. R of the template class R in (4, 8, 12) kept, x pass then y pass.
    kx, ky: (B, 25) as the record holds them.  mutant 'r8': a template of class 8 where 12 is due."""
    x = np.asarray(xp, np.float64)
    T = 8 if (mutant == "r8" and R == 12) else R
    out = np.zeros(x.shape)
    for b in range(x.shape[0]):
        hx, hy = np.zeros(KSIZE), np.zeros(KSIZE)
        hx[PAD - T:PAD + 1] = np.asarray(kx[b], np.float64)[PAD - T:PAD + 1]
        hy[PAD - T:PAD + 1] = np.asarray(ky[b], np.float64)[PAD - T:PAD + 1]
        hx[PAD:] = hx[PAD::-1]
        hy[PAD:] = hy[PAD::-1]
        out[b] = _apply(_apply(x[b], hx[None, :], boundary), hy[:, None], boundary)
    return out


def rank1_template(radius):
    return 4 if radius <= 4 else (8 if radius <= 8 else 12)


# ---------------------------------------------------------------------------------------------
# bounds
# ---------------------------------------------------------------------------------------------
def sum_bound(n_taps, S):
    """|got - want| per sample of an fp32 sum of n products in any order, with or without FMA: (n + 1) 2^-24 1.01 S + 1e-12"""
    return (n_taps + 1) * U32 * 1.01 * S + 1e-12


def half_ulp16(v):
    """half an fp16 ulp at the value v (normal range; at least the subnormal spacing)"""
    e = np.floor(np.log2(np.maximum(np.abs(v), 2.0 ** -14)))
    return 0.5 * 2.0 ** (e - 10)


# ---------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------
def white(shape, seed, dtype=np.float32):
    x = wr.flat(shape, seed).astype(dtype)
    x.setflags(write=False)
    return x


def _weights(rng, n):
    """n distinct weights of magnitude in [0.2, 1], signs mixed, scaled to sum 1"""
    w = rng.uniform(0.2, 1.0, n) * np.where(np.arange(n) % 3 == 1, -1.0, 1.0)
    if abs(w.sum()) < 0.3:
        w = np.abs(w)
    return w / w.sum()


# ---------------------------------------------------------------------------------------------
# family A: every tap position of every class
# ---------------------------------------------------------------------------------------------
A_SUPPORT = FULL | FORCE_GENERAL
A_SHAPE = (70, 76)                                  # 2 x 2 tiles, a pitch that is a multiple of 4


def a_positions(R):
    return [(i, j) for i in range(PAD - R, PAD + R + 1) for j in range(PAD - R, PAD + R + 1)]


@functools.lru_cache(maxsize=None)
def a_taps(R):
    """((2 R + 1)^2, 25, 25): 0.6 at (i, j), 0.4 at the anchor (12 - R, 12) that pins the class ((12 + R, 12) where (i, j) is it)"""
    pos = a_positions(R)
    k = np.zeros((len(pos), KSIZE, KSIZE), np.float32)
    for n, (i, j) in enumerate(pos):
        anchor = (PAD - R, PAD) if (i, j) != (PAD - R, PAD) else (PAD + R, PAD)
        k[n, anchor[0], anchor[1]] = 0.4
        k[n, i, j] = 0.6
    k.setflags(write=False)
    return k


def a_input(R):
    return white((len(a_positions(R)), 1) + A_SHAPE, 100 + R)


# ---------------------------------------------------------------------------------------------
# family B: the structures of the phase list (general body, forced)
# ---------------------------------------------------------------------------------------------
B_SUPPORT = FULL | FORCE_GENERAL


def b_columns(R):
    """the columns exactly one chunk of a class sees: (inner, first, last), indexed by kind"""
    inner = {4: 12, 6: 10, 8: 8, 10: 6, 12: 12}[R]
    return inner, PAD - R, PAD + R


# (inner, first, last) live phases: every pattern of empty / non-empty groups but all-empty, each group at an odd and at an even
# count, one live phase in all (three ways), a live phase in the list's last slot (every set whose last non-empty group is even)
B_COUNTS = ((1, 0, 0), (0, 1, 0), (0, 0, 1), (2, 0, 0), (0, 2, 0), (0, 0, 2), (1, 1, 0), (2, 2, 0), (1, 0, 1), (2, 0, 2),
            (0, 1, 1), (0, 2, 2), (1, 1, 1), (2, 2, 2), (3, 2, 1), (2, 1, 4), (4, 3, 2))


@functools.lru_cache(maxsize=None)
def b_cases(R):
    """-> [(name, taps (25, 25) fp32, claimed nphase)] of one class: the sparse sets of B_COUNTS, the class's full list (dense
    random, not point-symmetric) and the all-zero record (which has class 4 whatever R: listed under R = 4 only)"""
    cols = b_columns(R)
    out = []
    for ci, counts in enumerate(B_COUNTS):
        rng = np.random.default_rng(7000 + 100 * R + ci)
        k = np.zeros((KSIZE, KSIZE))
        w = iter(_weights(rng, sum(counts)))
        for kind, n in enumerate(counts):
            # (rows from the top of the box down for the first and the last column, which pin the class themselves; the inner
            # column starts at the box's first row, which pins it)
            rows = [PAD - R + 2 * t + kind for t in range(n)]
            for r in rows:
                k[r, cols[kind]] = next(w)
        out.append(("R%d-%d%d%d" % ((R,) + counts), k.astype(np.float32), [n + (n & 1) for n in counts]))
    rng = np.random.default_rng(7900 + R)
    box = rng.uniform(0.2, 1.0, (2 * R + 1, 2 * R + 1)) * np.where(rng.uniform(size=(2 * R + 1, 2 * R + 1)) < 0.3, -1.0, 1.0)
    k = np.zeros((KSIZE, KSIZE))
    k[PAD - R:PAD + R + 1, PAD - R:PAD + R + 1] = box / box.sum()
    n = 2 * R + 1
    full = [n * (R // 2 - 1), n, n]
    out.append(("R%d-full" % R, k.astype(np.float32), [c + (c & 1) for c in full]))
    if R == 4:
        out.append(("zero", np.zeros((KSIZE, KSIZE), np.float32), [0, 0, 0]))
    for _, k, _ in out:
        k.setflags(write=False)
    return out


B_SHAPE = (1, 70, 76)                               # (C, Hp, Wp) of a family B case


# ---------------------------------------------------------------------------------------------
# family C: the rank-1 body
# ---------------------------------------------------------------------------------------------
def _marginal(rng, r):
    """25 symmetric taps of radius r summing to 1, the odd offsets negative (none for r = 0); the centre tap at least 0.7 before
    scaling, the negative ones at most 0.2: the sum is at least 0.3"""
    h = np.zeros(KSIZE)
    v = rng.uniform(0.2, 1.0, r + 1) * np.where(np.arange(r + 1) % 2 == 1, -0.2, 1.0)
    v[0] = rng.uniform(0.7, 1.0)
    h[PAD:PAD + r + 1] = v
    h[PAD - r:PAD] = v[:0:-1]
    return h / h.sum()


# (rx, ry): every template class, radius 6 and below rounded up to 8, radius 10 up to 12, and the two extreme aspect ratios
C_RADII = ((4, 1), (1, 4), (5, 6), (6, 4), (8, 5), (5, 8), (9, 10), (10, 8), (12, 9), (12, 1), (1, 12), (0, 0))


@functools.lru_cache(maxsize=None)
def c_cases():
    """-> [(name, taps, claimed separable, claimed radius class of the record)]"""
    out = []
    for n, (rx, ry) in enumerate(C_RADII):
        rng = np.random.default_rng(8000 + n)
        k = np.outer(_marginal(rng, ry), _marginal(rng, rx)).astype(np.float32)
        rad = max(rx, ry)
        out.append(("rx%d-ry%d" % (rx, ry), k, 1, next(c for c in CLASSES if rad <= c)))
    rng = np.random.default_rng(8100)
    hx = _marginal(rng, 5)
    hx[PAD + 1:] *= 0.5                              # an asymmetric marginal: rank-1, but not the symmetrised factors' product
    k = np.outer(_marginal(rng, 3), hx / hx.sum()).astype(np.float32)
    out.append(("asymmetric-marginal", k, 0, 6))
    for _, k, _, _ in out:
        k.setflags(write=False)
    return out


C_SHAPE = (2, 70, 76)


# ---------------------------------------------------------------------------------------------
# family D: the tile-spectrum body (workgroup form): dense, point-symmetric, one per halo class
# (the GPU file runs them on a context created under PB_FFT_BODY=wg: by default a per-step pass takes the wave form)
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def d_taps(R):
    k = wr.dial_taps(R, R, False, 9000 + R)
    k.setflags(write=False)
    return k


D_SHAPE = (2, 70, 76)

# ---------------------------------------------------------------------------------------------
# family E: adaptive support
# ---------------------------------------------------------------------------------------------
# (theta deg, sigma, rho) whose radius class differs between the two policies: the taps underflow to zero far outside the box
# the marginals select
E_GAUSSIANS = ((30.0, 0.65, 0.40), (0.0, 0.6, 0.6), (66.0, 1.240, 0.625), (20.0, 0.9, 0.5))


def e_ring(value):
    """a caller kernel of class 8 (pinned by a cross of 0.01 at distance 8) with a 3 x 3 blob and a square ring of `value` at
    distance 6: at 5e-11 the ring's own chunks are dropped, at 2e-10 they are kept"""
    k = np.zeros((KSIZE, KSIZE))
    k[PAD - 1:PAD + 2, PAD - 1:PAD + 2] = np.array([[1, 2, 1], [2, 4, 2], [1, 2, 1]]) / 16.0 * 0.96
    for i, j in ((PAD - 8, PAD), (PAD + 8, PAD), (PAD, PAD - 8), (PAD, PAD + 8)):
        k[i, j] = 0.01
    for t in range(-6, 7):
        for i, j in ((PAD - 6, PAD + t), (PAD + 6, PAD + t), (PAD + t, PAD - 6), (PAD + t, PAD + 6)):
            k[i, j] = value
    k = k.astype(np.float32)
    k.setflags(write=False)
    return k


E_RINGS = (("ring-5e-11", 5e-11), ("ring-2e-10", 2e-10))
E_SHAPE = (1, 70, 76)

# ---------------------------------------------------------------------------------------------
# geometry: one record per body and class, both boundaries, both entry points
# ---------------------------------------------------------------------------------------------
GEOMETRY_BODIES = tuple(("general", R) for R in CLASSES) + tuple(("rank1", R) for R in RANK1_CLASSES) + \
    tuple(("spectrum", R) for R in RANK1_CLASSES)
SMALL_DOMAIN = (8, 9)                               # smaller than the support: wrap wraps more than once


def interior_pair(R, virtual=False):
    """the smallest square domain (padded sizes Hp x Wp; virtual: unpadded sizes of a virtual replicate-padded source) in which
    exactly one 64 x 64 tile of class R satisfies `inside` of load_tile (csrc/conv_tile_common.h), and the one a row smaller in
    which none does.  Tile (ty, tx) stages rows 64 ty - R .. 64 ty + 64 + R of the padded domain: inside it from ty = 1 on, where
    64 + 64 + R <= Hp; a virtual source also asks for 64 ty - R >= 12 and 64 ty + 64 + R <= 12 + H."""
    n = 128 + R - (PAD if virtual else 0)
    assert _inside_tiles(n, n, R, virtual) == 1 and _inside_tiles(n - 1, n, R, virtual) == 0 and _inside_tiles(n, n - 1, R, virtual) == 0
    return (n, n), (n - 1, n)


def _inside_tiles(h, w, R, virtual):
    """how many tiles of an h x w domain (virtual: unpadded sizes; the output is the padded domain) satisfy `inside`"""
    H, W = (h, w) if virtual else (h - 2 * PAD, w - 2 * PAD)
    Hp, Wp = H + 2 * PAD, W + 2 * PAD
    L, count = 64 + 2 * R, 0
    for ty in range((Hp + 63) // 64):
        for tx in range((Wp + 63) // 64):
            py0, px0 = 64 * ty - R, 64 * tx - R
            ok = py0 >= 0 and px0 >= 0 and py0 + L <= Hp and px0 + L <= Wp
            if virtual:
                ok = ok and py0 >= PAD and px0 >= PAD and py0 + L <= PAD + H and px0 + L <= PAD + W
            count += ok
    return count


def convolve_domains(R):
    """the Hp x Wp domains of pb_convolve2d for a record of class R"""
    return [(64, 64), (65, 68), (67, 131)] + list(interior_pair(R))


def inverse_shapes(R):
    """the H x W images of pb_inverse_filter: the unpadded sizes that give convolve_domains' tiles, and the virtual-source pair"""
    return [(h - 2 * PAD, w - 2 * PAD) for h, w in convolve_domains(R)] + list(interior_pair(R, virtual=True))


def fp16_shapes(R):
    s = sorted(inverse_shapes(R), key=lambda hw: hw[0] * hw[1])
    return s[:2] + s[-2:]


@functools.lru_cache(maxsize=None)
def geometry_taps(body, R):
    """the record of one body and class.  general: 9 taps that pin the class, one in each kind of chunk among them, not
    point-symmetric; rank1: symmetric marginals of radius R and R - 1; spectrum: family D's."""
    if body == "spectrum":
        return d_taps(R)
    rng = np.random.default_rng(9500 + R + (100 if body == "rank1" else 0))
    if body == "rank1":
        k = np.outer(_marginal(rng, R - 1), _marginal(rng, R)).astype(np.float32)
    else:
        inner, first, last = b_columns(R)
        pos = [(PAD - R, inner), (PAD - R + 1, first), (PAD + R, last), (PAD, PAD), (PAD + 1, PAD - 2), (PAD - 2, PAD + 3),
               (PAD + R - 1, PAD + 1), (PAD - 1, first), (PAD + 2, last)]
        k = np.zeros((KSIZE, KSIZE))
        w = rng.uniform(0.2, 1.0, len(pos))         # (positive: the polynomial of a kernel with |K^| <= 1 keeps white input in range)
        for (i, j), v in zip(pos, w / w.sum()):
            k[i, j] = v
        k = k.astype(np.float32)
    k.setflags(write=False)
    return k


def geometry_support(body):
    return FULL | FORCE_GENERAL if body == "general" else FULL


def geometry_pair(body, R):
    """the records of the two images of a geometry batch: this body's and the next class's of the same body (wrapping round)"""
    cls = CLASSES if body == "general" else RANK1_CLASSES
    other = cls[(cls.index(R) + 1) % len(cls)]
    return np.stack([geometry_taps(body, R), geometry_taps(body, other)])


GEOMETRY_COEF = (wr.ALPHA, wr.BETA)
