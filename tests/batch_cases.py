"""Many-job launches of the batched entry points of include/x265hip.h: the case tables of tests/test_batch_launches.py.

A Case is one launch, described without any GPU import: the host arrays to upload (`bufs`), which of them the launch writes
(`outs`), the argument list of the C entry point (Buf(name) marks a device pointer) and three views of the expected result:

  oracle()   the pinned oracle (oracle/pyoracle.py, backends.Orc) called once per job, its results placed into copies of the
             sentinel-filled output buffers — so one array comparison checks the jobs' cells AND everything around them;
  restate()  the same in a few lines of int64 numpy, vectorised over the jobs, where the operation has such a restatement
             (restate(mut=...) applies one of the batching faults the issue lists, for the mutation check of the CPU tier);
  cells      a bool mask per output: the elements the jobs own.  Everything else must still hold the sentinel after the launch.

Every table obeys the same rules: offsets distinct per job and shuffled (not monotone in the job index), origins at odd x,
sources free to overlap, destinations disjoint with a guard band around each block, all pitches of a launch different from each
other and from the block width, dense outputs with GUARD_ROWS sentinel rows behind job n - 1."""
import numpy as np

from backends import Orc
from oracle import pyoracle as po

def ptr(a, y=0, x=0):
    return po.ptr(a, int(y), int(x))


def at(ys, xs, i):
    return int(ys[i]), int(xs[i])


NS = (7, 67, 530)                  # the job counts of test_hip_parity.test_transform_batches
DEPTHS = (8, 10, 12)
GUARD_ROWS = 8
# grid_for()'s default cap in x265_amd/csrc/common.h: 256 * 16 workgroups of 256 lanes (4 waves); launches that need more loop grid-stride
GRID_CAP_WORKGROUPS = 256 * 16
LANES_PER_WORKGROUP = 256
IF_KINDS = {"hpp": 0, "hps": 1, "vpp": 2, "vps": 3, "vsp": 4, "vss": 5, "hvpp": 6}     # X265HIP_IF_* of include/x265hip.h


def sentinel(dtype):
    return np.frombuffer(b"\xa5" * 8, np.dtype(dtype))[0]


def filled(shape, dtype):
    return np.full(shape, sentinel(dtype), dtype)


class Buf:
    """A device-pointer argument: the upload of Case.bufs[name]."""
    def __init__(self, name):
        self.name = name


class Case:
    def __init__(self, fn, entry, shape, n, depth, bufs, outs, args, cells, job=None, oracle=None, restate=None, big=False, offsets=(), pitches=(), width=0, guarded=True, witness=None):
        self.fn, self.entry, self.shape, self.n, self.depth = fn, entry, shape, n, depth
        self.bufs, self.outs, self.args, self.cells = bufs, outs, args, cells
        self._job, self._oracle, self.restate, self.big = job, oracle, restate, big
        self.offsets, self.pitches, self.width = offsets, pitches, width        # what the CPU tier checks the builder on
        self.guarded = guarded          # False: the jobs' cells abut, as the units of one edge do in a picture
        self.witness = witness or (lambda want: {})     # want -> what the CPU tier must see reached; computes, changes nothing

    @property
    def label(self):
        return "%s %s n=%d depth=%s" % (self.entry, self.shape, self.n, self.depth)

    def placements(self, jobs):
        """[(out name, index, value)] of the oracle for the given jobs."""
        o = Orc(self.depth or 8)
        return [p for i in jobs for p in self._job(o, i)]

    def oracle(self):
        if self._oracle:
            return self._oracle()
        out = {k: self.bufs[k].copy() for k in self.outs}
        for k, idx, val in self.placements(range(self.n)):
            out[k][idx] = val
        return out

    def want(self):
        """What the launch must leave: the oracle per job; for the launches past the grid cap the numpy restatement (spot-checked by the oracle in the CPU tier)."""
        return self.restate() if self.big else self.oracle()


# ---- placing jobs --------------------------------------------------------------------------------------------------------------
def _idx(ys, xs, h, w):
    return ys[:, None, None] + np.arange(h)[None, :, None], xs[:, None, None] + np.arange(w)[None, None, :]


def gather(plane, ys, xs, h, w):
    """[n, h, w] int64 copies of the (overlapping) blocks at (ys, xs)."""
    r, c = _idx(ys, xs, h, w)
    return plane[r, c].astype(np.int64)


def scatter(dst, ys, xs, blocks):
    r, c = _idx(ys, xs, blocks.shape[1], blocks.shape[2])
    dst[r, c] = blocks.astype(dst.dtype)        # a C cast: wraps like (pixel)v


def block_mask(shape, ys, xs, h, w):
    m = np.zeros(shape, bool)
    r, c = _idx(ys, xs, h, w)
    m[r, c] = True
    return m


def dense_mask(shape, n):
    m = np.zeros(shape, bool)
    m[:n] = True
    return m


def chunks(n, step=2048):
    return [slice(i, min(n, i + step)) for i in range(0, n, step)]


def shuffled(rng, pick):
    """`pick` (distinct slot numbers) in an order that is not monotone, whatever the draw"""
    while len(pick) > 2 and (np.all(np.diff(pick) > 0) or np.all(np.diff(pick) < 0)):
        pick = rng.permutation(pick)
    return pick


def src_origins(rng, n, ny, nx, y0=0, x0=1):
    """n distinct origins in shuffled order, x odd: blocks overlap freely."""
    pick = shuffled(rng, rng.choice(ny * nx, n, replace=False))
    return y0 + pick // nx, x0 + 2 * (pick % nx)


def dst_grid(rng, n, w, h, avoid=()):
    """Disjoint w x h cells in shuffled order, x odd, one guard row and two guard columns between neighbours and around the lot.
    Returns (ys, xs, plane shape); the pitch differs from every pitch in `avoid` and from w."""
    cols = int(np.ceil(np.sqrt(n)))
    rows = -(-n // cols)
    slot = shuffled(rng, rng.permutation(rows * cols)[:n])
    W = cols * (w + 2) + 1
    while W in avoid or W == w:
        W += 2
    return 1 + (slot // cols) * (h + 1), 1 + (slot % cols) * (w + 2), (rows * (h + 1) + 2, W)


def flat(ys, xs, plane):
    return (ys * plane.shape[1] + xs).astype(np.int32)


def operand(rng, kind, shape, depth):
    """p: pixels; r: residuals -pmax .. pmax; a: the 14-bit intermediate -8192 .. 8191; w: all of int16 but -32768.  Each with both rails frequent."""
    pmax = (1 << depth) - 1
    lo, hi = {"p": (0, pmax), "r": (-pmax, pmax), "a": (-8192, 8191), "w": (-32767, 32767)}[kind]
    v = rng.integers(lo, hi + 1, shape)
    u = rng.random(shape)
    v[u < 0.08] = lo
    v[u > 0.92] = hi
    return v.astype(po.pix_dtype(depth) if kind == "p" else np.int16)


# ---- family 2: the elementwise kernel --------------------------------------------------------------------------------------------
# entry: (ABI name, leading kind argument, dst / src0 / src1 element kinds, order of the (plane, pitch) pairs and of the offset arrays)
EW_ENTRIES = {
    "sub_ps": ("x265hip_sub_ps_batch", None, "s", "p", "p", "D01"),
    "add_ps": ("x265hip_add_ps_batch", None, "p", "p", "r", "D01"),
    "addavg": ("x265hip_addavg_batch", None, "p", "a", "a", "01D"),
    "pixelavg_pp": ("x265hip_pixelavg_pp_batch", None, "p", "p", "p", "D01"),
    "copy_pp": ("x265hip_copy_batch", 0, "p", "p", None, "D0"),
    "copy_sp": ("x265hip_copy_batch", 1, "p", "r", None, "D0"),
    "copy_ps": ("x265hip_copy_batch", 2, "s", "p", None, "D0"),
    "copy_ss": ("x265hip_copy_batch", 3, "s", "r", None, "D0"),
    "p2s": ("x265hip_p2s_batch", None, "s", "p", None, "0D"),
}
EW_SHAPES = [(2, 4), (6, 8), (4, 4), (12, 16), (24, 32), (64, 64)]     # every ew entry admits valid_block(): 2x4 and 6x8 take the V = 2 form


def np_ew(entry, depth, a, b):
    pmax = (1 << depth) - 1
    if entry == "sub_ps":
        return a - b
    if entry == "add_ps":
        return np.clip(a + b, 0, pmax)
    if entry == "addavg":
        shift = 14 + 1 - depth
        return np.clip((a + b + (1 << (shift - 1)) + 2 * 8192) >> shift, 0, pmax)
    if entry == "pixelavg_pp":
        return (a + b + 1) >> 1
    if entry == "p2s":
        return (a << (14 - depth)) - 8192
    return a


def orc_ew(o, entry, w, h, a, ao, b, bo):
    d = np.zeros((h, w), np.int16 if EW_ENTRIES[entry][2] == "s" else o.pix)
    pa, sa = ptr(a, *ao), a.shape[1]
    pb, sb = (ptr(b, *bo), b.shape[1]) if b is not None else (None, 0)
    if entry == "sub_ps":
        o._f("orc_sub_ps")(ptr(d), w, pa, pb, sa, sb, w, h)
    elif entry == "add_ps":
        o._f("orc_add_ps")(ptr(d), w, pa, pb, sa, sb, w, h, o.depth)
    elif entry == "addavg":
        o._f("orc_addAvg")(pa, pb, ptr(d), sa, sb, w, w, h, o.depth)
    elif entry == "pixelavg_pp":
        o._f("orc_pixelavg_pp")(ptr(d), w, pa, sa, pb, sb, w, h)
    elif entry == "p2s":
        o._f("orc_p2s")(pa, sa, ptr(d), w, w, h, o.depth)
    elif entry == "copy_ss":
        o.L.orc_copy_ss(ptr(d), w, pa, sa, w, h)
    else:
        o._f("orc_" + entry)(ptr(d), w, pa, sa, w, h)
    return d


def ew_case(entry, depth, w, h, n, seed, ny=24, nx=24, big=False):
    fn, kind, kd, k0, k1, order = EW_ENTRIES[entry]
    rng = np.random.default_rng(seed)
    S0 = operand(rng, k0, (h + ny, w + 2 * nx + 1), depth)
    y0, x0 = src_origins(rng, n, ny, nx)
    S1 = operand(rng, k1, (h + ny + 2, w + 2 * nx + 7), depth) if k1 else None
    y1, x1 = src_origins(rng, n, ny, nx) if k1 else (None, None)
    dy, dx, dshape = dst_grid(rng, n, w, h, avoid=(S0.shape[1], w + 2 * nx + 7))
    D = filled(dshape, np.int16 if kd == "s" else po.pix_dtype(depth))
    bufs = {"D": D, "S0": S0, "oD": flat(dy, dx, D), "o0": flat(y0, x0, S0)}
    if k1:
        bufs.update({"S1": S1, "o1": flat(y1, x1, S1)})
    names = {"D": ("D", "oD"), "0": ("S0", "o0"), "1": ("S1", "o1")}
    args = ([kind] if kind is not None else []) + [depth, w, h]
    for ch in order:
        args += [Buf(names[ch][0]), bufs[names[ch][0]].shape[1]]
    args += [Buf(names[ch][1]) for ch in order] + [n, None]

    def job(o, i):
        return [("D", (slice(dy[i], dy[i] + h), slice(dx[i], dx[i] + w)),
                 orc_ew(o, entry, w, h, S0, at(y0, x0, i), S1, at(y1, x1, i) if k1 else None))]

    def restate(mut=None):
        first = lambda v: np.full(n, v[0])                  # noqa: E731 - the fault: every job uses job 0's offset
        sy, sx = (first(y0), first(x0)) if mut == "off0[0]" else (y0, x0)
        ty, tx = (first(dy), first(dx)) if mut == "offD[0]" else (dy, dx)
        out = D.copy()
        for s in chunks(n, 8192):
            scatter(out, ty[s], tx[s], np_ew(entry, depth, gather(S0, sy[s], sx[s], h, w), gather(S1, y1[s], x1[s], h, w) if k1 else None))
        return {"D": out}

    def witness(want):
        if entry != "add_ps":
            return {}
        v = gather(S0, y0, x0, h, w) + gather(S1, y1, x1, h, w)
        return {"clips_low": bool((v < 0).any()), "clips_high": bool((v > (1 << depth) - 1).any())}

    c = Case(fn, entry, "%dx%d" % (w, h), n, depth, bufs, ["D"], args, {"D": block_mask(D.shape, dy, dx, h, w)}, job=job, restate=restate, big=big, witness=witness,
             offsets=[(bufs["o" + k[-1]], bufs[k].shape[1]) for k in ("D", "S0", "S1") if k in bufs], pitches=[bufs[k].shape[1] for k in ("D", "S0", "S1") if k in bufs], width=w)
    return c


# ---- family 1: the wave-packed kernels ---------------------------------------------------------------------------------------------
WAVE_SHAPES = [(4, 4), (8, 4), (8, 8), (12, 16), (16, 16), (24, 32), (32, 32), (64, 64)]
SQUARE = [4, 8, 16, 32, 64]


def jobs_per_wave(w, h):
    """bpw of pixcmp_kernel / sse_kernel (x265_amd/csrc/pixel.hip): T = min(64, pow2_ceil(tiles)) lanes share a block."""
    tiles = (w // 4) * (h // 4)
    T = 1
    while T < min(tiles, 64):
        T *= 2
    return 64 // T


def wave_counts(w, h):
    """one job more than a wave holds; two full workgroups (4 waves each) and a ragged wave of a third"""
    b = jobs_per_wave(w, h)
    return (b + 1, 8 * b + 3)


def sse_case(entry, depth, w, h, n, seed, ny=24, nx=24, big=False):
    """entry sse_pp (pixels), sse_ss (int16), ssd_s (int16, planeB == NULL).  Two rail jobs ride in every launch: all-high against all-zero and
    high against low rail (pmax / 0 for pixels, +-32767 for int16), as the last job and a middle one."""
    rng = np.random.default_rng(seed)
    k = "p" if entry == "sse_pp" else "w"
    hi, lo = ((1 << depth) - 1, 0) if k == "p" else (32767, -32767)
    W = max(w + 2 * nx + 1, 2 * w + 5)
    A, B = operand(rng, k, (ny + 2 * h, W), depth or 8), operand(rng, k, (ny + 2 * h + 1, W + 6), depth or 8)
    A[ny + h:, 1:1 + w], B[ny + h:, 1:1 + w] = hi, 0
    A[ny + h:, w + 3:2 * w + 3], B[ny + h:, w + 3:2 * w + 3] = (lo, hi) if k == "p" else (hi, lo)
    ya, xa = src_origins(rng, n, ny, nx)
    yb, xb = src_origins(rng, n, ny, nx)
    if not big:
        for j, x in ((n - 1, 1), ((n - 1) // 2, w + 3)):
            ya[j], xa[j], yb[j], xb[j] = ny + h, x, ny + h, x
    out = filled(n + GUARD_ROWS, np.uint64)
    zeros = np.zeros((h, w), np.int16)
    bufs = {"A": A, "oA": flat(ya, xa, A), "out": out}
    if entry == "ssd_s":
        args = [w, h, Buf("A"), A.shape[1], None, 0, Buf("oA"), None, n, Buf("out"), None]
    else:
        bufs.update({"B": B, "oB": flat(yb, xb, B)})
        args = ([depth] if entry == "sse_pp" else []) + [w, h, Buf("A"), A.shape[1], Buf("B"), B.shape[1], Buf("oA"), Buf("oB"), n, Buf("out"), None]

    def job(o, i):
        if entry == "sse_pp":
            v = o._f("orc_sse_pp")(ptr(A, ya[i], xa[i]), A.shape[1], ptr(B, yb[i], xb[i]), B.shape[1], w, h)
        elif entry == "sse_ss":
            v = o.L.orc_sse_ss(ptr(A, ya[i], xa[i]), A.shape[1], ptr(B, yb[i], xb[i]), B.shape[1], w, h)
        elif w == h:
            v = o.L.orc_ssd_s(ptr(A, ya[i], xa[i]), A.shape[1], w)
        else:                                       # cu[].ssd_s is square in the reference; elsewhere sse_ss against zeros is the same sum
            v = o.L.orc_sse_ss(ptr(A, ya[i], xa[i]), A.shape[1], ptr(zeros), w, w, h)
        return [("out", i, v)]

    def restate(mut=None):
        r = out.copy()
        for s in chunks(n):
            z = np.zeros(s.stop - s.start, np.int64)
            a = gather(A, ya[s], xa[s], h, w) if mut != "offA[0]" else gather(A, z + ya[0], z + xa[0], h, w)
            d = a - gather(B, yb[s], xb[s], h, w) if entry != "ssd_s" else a
            r[s] = (d * d).sum(axis=(1, 2)).astype(np.uint64)
        if mut == "tail lanes write":        # jobOk dropped from the final store: the clamped lanes store job n - 1's sum behind it
            b = jobs_per_wave(w, h)
            r[n:-(-n // b) * b] = r[n - 1]
        return {"out": r}

    def witness(want):
        return {"above_2^32": bool((want["out"][:n] > np.uint64(1 << 32)).any())}

    c = Case("x265hip_sse_pp_batch" if entry == "sse_pp" else "x265hip_sse_ss_batch", entry, "%dx%d" % (w, h), n, depth, bufs, ["out"], args,
             {"out": dense_mask(out.shape, n)}, job=job, restate=restate, big=big, witness=witness, offsets=[(bufs["o" + x], bufs[x].shape[1]) for x in ("A", "B") if x in bufs],
             pitches=[A.shape[1]] + ([B.shape[1]] if entry != "ssd_s" else []), width=w)
    return c


def sad_xn_case(K, depth, w, h, n, seed, ny=24, nx=24, big=False):
    """Every job its own source block, every candidate its own unrelated reference block; out [n][K]."""
    rng = np.random.default_rng(seed)
    ny = nx = max(ny, int(np.ceil(np.sqrt(n * K))))        # n * K distinct reference origins
    F, R = operand(rng, "p", (ny + h, w + 2 * nx + 1), depth), operand(rng, "p", (ny + h + 3, w + 2 * nx + 9), depth)
    yf, xf = src_origins(rng, n, ny, nx)
    yr, xr = src_origins(rng, n * K, ny, nx)
    out = filled((n + GUARD_ROWS, K), np.int32)
    bufs = {"F": F, "R": R, "oF": flat(yf, xf, F), "oR": flat(yr, xr, R), "out": out}
    args = [K, depth, w, h, Buf("F"), F.shape[1], Buf("R"), R.shape[1], Buf("oF"), Buf("oR"), n, Buf("out"), None]

    def job(o, i):
        fenc = np.zeros((64, 64), o.pix)           # the reference's sad_x3 / sad_x4 read the source block at FENC_STRIDE = 64
        fenc[:h, :w] = F[yf[i]:yf[i] + h, xf[i]:xf[i] + w]
        return [("out", i, o.sad_xn(w, h, fenc, R, [(int(yr[i * K + k]), int(xr[i * K + k])) for k in range(K)]))]

    def restate(mut=None):
        r = out.copy()
        for s in chunks(n, 1024):
            z = np.zeros(s.stop - s.start, np.int64)
            f = gather(F, yf[s], xf[s], h, w) if mut != "offF[0]" else gather(F, z + yf[0], z + xf[0], h, w)
            for k in range(K):
                r[s, k] = np.abs(f - gather(R, yr[k::K][s], xr[k::K][s], h, w)).sum(axis=(1, 2))
        return {"out": r}

    return Case("x265hip_sad_xn_batch", "sad_x%d" % K, "%dx%d" % (w, h), n, depth, bufs, ["out"], args, {"out": dense_mask(out.shape, n)}, job=job,
                restate=restate, big=big, offsets=[(bufs["oF"], F.shape[1]), (bufs["oR"], R.shape[1])], pitches=[F.shape[1], R.shape[1]], width=w)


# ---- family 3: one launch past the grid cap per kernel, depth 8 ------------------------------------------------------------------------
def past_the_cap_cases():
    """ew_kernel: one lane makes V elements and the grid holds GRID_CAP_WORKGROUPS * 256 lanes, so the second trip starts at more than 1 048 576 lanes —
    2 097 154 elements at a V = 2 shape, twice that at a V = 4 shape (1 025 jobs of 64x64).  6x8 is the V = 2 shape with the fewer jobs (24 lanes a job).
    sse_kernel / pixcmp_kernel: a wave takes 64 / T jobs a trip and the grid holds 4 * GRID_CAP_WORKGROUPS waves, so the second trip needs more than
    16 384 wave-loads; a full wave-load is 1 024 elements at every shape but 64x64 (4 096), and 32x32 is the shape with one job a wave — the fewest jobs
    (16 385, a quarter of the elements of 16 385 jobs of 64x64).  sad_x4 reaches it with n * 4 > 16 384 kernel jobs."""
    lanes = GRID_CAP_WORKGROUPS * LANES_PER_WORKGROUP
    waves = GRID_CAP_WORKGROUPS * (LANES_PER_WORKGROUP // 64)
    n_ew = lanes // ((6 // 2) * 8) + 1
    n_wave = waves // jobs_per_wave(32, 32) + 1
    assert n_ew == 43691 and n_wave == 16385
    return [ew_case("sub_ps", 8, 6, 8, n_ew, 9001, ny=210, nx=210, big=True),
            sse_case("sse_pp", 8, 32, 32, n_wave, 9002, ny=130, nx=130, big=True),
            sad_xn_case(4, 8, 32, 32, n_wave // 4 + 1, 9003, ny=130, nx=130, big=True)]


# ---- family 4: quantisation, denoise, the 4x4 DST -----------------------------------------------------------------------------------------
def nquant_case(size, n, seed):
    rng = np.random.default_rng(seed)
    nc, log2n = size * size, size.bit_length() - 1
    coef = operand(rng, "w", (n, nc), 8) // 40
    units = rng.permutation(n)
    coef[units[:2]] = rng.integers(-2, 3, (2, nc))                                    # nothing survives: numSig 0
    coef[units[2:4]] = rng.integers(3000, 32768, (2, nc)) * rng.choice([-1, 1], (2, nc))    # everything does: numSig numCoeff
    qc = rng.integers(14000, 27000, nc).astype(np.int32)
    qbits = 14 + 27 // 6 + (15 - 8 - log2n)
    add = 171 << (qbits - 9)
    q, ns = filled((n + GUARD_ROWS, nc), np.int16), filled(n + GUARD_ROWS, np.uint32)
    bufs = {"coef": coef, "qc": qc, "q": q, "ns": ns}
    args = [Buf("coef"), Buf("qc"), Buf("q"), qbits, add, nc, n, Buf("ns"), None]

    def job(o, i):
        lv, cnt = o.nquant(coef[i], qc, qbits, add)
        return [("q", i, lv), ("ns", i, cnt)]

    def restate(mut=None):
        c64 = coef.astype(np.int64)
        lv = (np.abs(c64) * qc + add) >> qbits
        rq, rn = q.copy(), ns.copy()
        rn[:n] = (lv != 0).sum(axis=1)
        rq[:n] = np.abs(np.clip(lv * np.where(c64 < 0, -1, 1), -32768, 32767))
        return {"q": rq, "ns": rn}

    def witness(want):
        return {"numSig_0": bool((want["ns"][:n] == 0).any()), "numSig_all": bool((want["ns"][:n] == nc).any())}

    c = Case("x265hip_nquant_batch", "nquant", "%dx%d" % (size, size), n, None, bufs, ["q", "ns"], args, {"q": dense_mask(q.shape, n), "ns": dense_mask(ns.shape, n)},
             job=job, restate=restate, witness=witness)
    return c


def dequant_scaling_case(size, n, per, shift, seed):
    rng = np.random.default_rng(seed)
    nc = size * size
    q = operand(rng, "w", (n, nc), 8)
    q[:, ::3] //= 64
    dqc = rng.integers(16, 1200, nc).astype(np.int32)                                  # non-flat; |q * dqc| < 2^26
    out = filled((n + GUARD_ROWS, nc), np.int16)
    bufs = {"q": q, "dqc": dqc, "out": out}
    args = [Buf("q"), Buf("dqc"), Buf("out"), nc, n, per, shift, None]

    def job(o, i):
        return [("out", i, o.dequant_scaling(q[i], dqc, per, shift))]

    def unclipped():
        s, p = shift + 4, q.astype(np.int64) * dqc
        return (p + (1 << (s - per - 1))) >> (s - per) if s > per else np.clip(p, -32768, 32767) << (per - s)

    def restate(mut=None):
        r = out.copy()
        r[:n] = np.clip(unclipped(), -32768, 32767)
        return {"out": r}

    def witness(want):
        v = unclipped()
        return {"branch": "shift>per" if shift + 4 > per else "shift<=per", "saturates": bool((v < -32768).any() and (v > 32767).any())}

    c = Case("x265hip_dequant_scaling_batch", "dequant_scaling", "%dx%d per%d shift%d" % (size, size, per, shift), n, None, bufs, ["out"], args,
             {"out": dense_mask(out.shape, n)}, job=job, restate=restate, witness=witness)
    return c


def denoise_case(size, n, seed):
    """dctCoef in place, resSum shared by the n units: it starts non-zero and must end at start + the sum over all units."""
    rng = np.random.default_rng(seed)
    nc = size * size
    coef = filled((n + GUARD_ROWS, nc), np.int16)
    coef[:n] = operand(rng, "w", (n, nc), 8) // 64
    coef[:n:5] = operand(rng, "w", coef[:n:5].shape, 8)
    res = filled(nc + GUARD_ROWS, np.uint32)
    res[:nc] = rng.integers(1, 1 << 31, nc)
    offset = rng.integers(0, 400, nc).astype(np.uint16)
    bufs = {"coef": coef, "res": res, "offset": offset}
    args = [Buf("coef"), Buf("res"), Buf("offset"), nc, n, None]

    def oracle():
        o = Orc(8)
        cf, r = coef.copy(), res.copy()
        acc = r[:nc].copy()
        for i in range(n):
            cf[i], acc = o.denoise_dct(cf[i], acc, offset)
        r[:nc] = acc
        return {"coef": cf, "res": r}

    def restate(mut=None):
        a = np.abs(coef[:n].astype(np.int64))
        cf, r = coef.copy(), res.copy()
        total = a.sum(axis=0) if mut != "resSum of one unit" else a[n - 1]
        r[:nc] = (res[:nc].astype(np.int64) + total) & 0xffffffff
        lv = a - offset
        cf[:n] = np.where(lv < 0, 0, lv * np.sign(coef[:n]))
        return {"coef": cf, "res": r}

    def witness(want):
        zeroed = (coef[:n] != 0) & (np.abs(coef[:n].astype(np.int64)) < offset)
        return {"zeroed": bool(zeroed.any()), "resSum_changes": bool((want["res"][:nc] != res[:nc]).any()), "start_nonzero": bool(res[:nc].all())}

    c = Case("x265hip_denoise_dct_batch", "denoise_dct", "%dx%d" % (size, size), n, None, bufs, ["coef", "res"], args,
             {"coef": dense_mask(coef.shape, n), "res": dense_mask(res.shape, nc)}, oracle=oracle, restate=restate, witness=witness)
    return c


def dst4_case(depth, n, inverse, seed, ny=24, nx=24):
    rng = np.random.default_rng(seed)
    if not inverse:
        plane = operand(rng, "r", (4 + ny, 4 + 2 * nx + 1), depth)
        ys, xs = src_origins(rng, n, ny, nx)
        out = filled((n + GUARD_ROWS, 16), np.int16)
        bufs = {"src": plane, "off": flat(ys, xs, plane), "out": out}
        args = [4, 1, depth, Buf("src"), plane.shape[1], Buf("off"), Buf("out"), n, None]

        def job(o, i):
            return [("out", i, o.dst4(plane, at(ys, xs, i)))]
        return Case("x265hip_dct_batch", "dst4", "4x4", n, depth, bufs, ["out"], args, {"out": dense_mask(out.shape, n)}, job=job, offsets=[(bufs["off"], plane.shape[1])],
                    pitches=[plane.shape[1]], width=4)
    coef = operand(rng, "w", (n, 16), depth)
    coef[::2] //= 16
    dy, dx, dshape = dst_grid(rng, n, 4, 4)
    D = filled(dshape, np.int16)
    bufs = {"coef": coef, "D": D, "off": flat(dy, dx, D)}
    args = [4, 1, depth, Buf("coef"), Buf("D"), D.shape[1], Buf("off"), n, None]

    def job(o, i):
        return [("D", (slice(dy[i], dy[i] + 4), slice(dx[i], dx[i] + 4)), o.idst4(coef[i]))]
    return Case("x265hip_idct_batch", "idst4", "4x4", n, depth, bufs, ["D"], args, {"D": block_mask(D.shape, dy, dx, 4, 4)}, job=job, offsets=[(bufs["off"], D.shape[1])],
                pitches=[D.shape[1]], width=4)


# ---- family 5: var, transpose, the two downscales -------------------------------------------------------------------------------------------
def var_case(depth, size, n, seed, ny=24, nx=24):
    """One job of every launch is an all-pmax block (at 12 bit and 64x64 the sum of squares wraps 32 bits, as the reference's does)."""
    rng = np.random.default_rng(seed)
    plane = operand(rng, "p", (ny + 2 * size, max(size + 2 * nx + 1, size + 3)), depth)
    plane[ny + size:, 1:1 + size] = (1 << depth) - 1
    ys, xs = src_origins(rng, n, ny, nx)
    ys[n // 2], xs[n // 2] = ny + size, 1
    out = filled(n + GUARD_ROWS, np.uint64)
    bufs = {"plane": plane, "off": flat(ys, xs, plane), "out": out}
    args = [depth, size, Buf("plane"), plane.shape[1], Buf("off"), n, Buf("out"), None]

    def job(o, i):
        return [("out", i, o.var(size, plane, at(ys, xs, i)))]
    return Case("x265hip_var_batch", "var", "%dx%d" % (size, size), n, depth, bufs, ["out"], args, {"out": dense_mask(out.shape, n)}, job=job, offsets=[(bufs["off"], plane.shape[1])],
                pitches=[plane.shape[1]], width=size)


def transpose_case(depth, size, n, seed, ny=24, nx=24):
    rng = np.random.default_rng(seed)
    plane = operand(rng, "p", (ny + size, size + 2 * nx + 1), depth)
    ys, xs = src_origins(rng, n, ny, nx)
    out = filled((n + GUARD_ROWS, size * size), plane.dtype)
    bufs = {"plane": plane, "off": flat(ys, xs, plane), "out": out}
    args = [depth, size, Buf("plane"), plane.shape[1], Buf("off"), Buf("out"), n, None]

    def job(o, i):
        return [("out", i, o.transpose(size, plane, at(ys, xs, i)).reshape(-1))]

    def restate(mut=None):
        r = out.copy()
        r[:n] = gather(plane, ys, xs, size, size).swapaxes(1, 2).reshape(n, -1)
        return {"out": r}
    return Case("x265hip_transpose_batch", "transpose", "%dx%d" % (size, size), n, depth, bufs, ["out"], args, {"out": dense_mask(out.shape, n)}, job=job, restate=restate,
                offsets=[(bufs["off"], plane.shape[1])], pitches=[plane.shape[1]], width=size)


def scale1d_case(depth, n, seed):
    rng = np.random.default_rng(seed)
    src = operand(rng, "p", (n, 256), depth)
    out = filled((n + GUARD_ROWS, 128), src.dtype)
    bufs = {"src": src, "out": out}

    def job(o, i):
        return [("out", i, o.scale1d_128to64(src[i]))]

    def restate(mut=None):
        r, s = out.copy(), src.astype(np.int64)
        r[:n] = (s[:, 0::2] + s[:, 1::2] + 1) >> 1
        return {"out": r}
    return Case("x265hip_scale1d_128to64_batch", "scale1d_128to64", "128+128", n, depth, bufs, ["out"], [depth, Buf("src"), Buf("out"), n, None],
                {"out": dense_mask(out.shape, n)}, job=job, restate=restate)


def scale2d_case(depth, n, seed, ny=24, nx=24):
    rng = np.random.default_rng(seed)
    plane = operand(rng, "p", (ny + 64, 64 + 2 * nx + 1), depth)
    ys, xs = src_origins(rng, n, ny, nx)
    out = filled((n + GUARD_ROWS, 1024), plane.dtype)
    bufs = {"plane": plane, "off": flat(ys, xs, plane), "out": out}

    def job(o, i):
        return [("out", i, o.scale2d_64to32(plane, at(ys, xs, i)).reshape(-1))]

    def restate(mut=None):
        r, a = out.copy(), gather(plane, ys, xs, 64, 64)
        r[:n] = ((a[:, 0::2, 0::2] + a[:, 0::2, 1::2] + a[:, 1::2, 0::2] + a[:, 1::2, 1::2] + 2) >> 2).reshape(n, -1)
        return {"out": r}
    return Case("x265hip_scale2d_64to32_batch", "scale2d_64to32", "64x64", n, depth, bufs, ["out"], [depth, Buf("plane"), plane.shape[1], Buf("off"), Buf("out"), n, None],
                {"out": dense_mask(out.shape, n)}, job=job, restate=restate, offsets=[(bufs["off"], plane.shape[1])], pitches=[plane.shape[1]], width=64)


# ---- family 6: intra neighbour filter, all angular modes ----------------------------------------------------------------------------------------
def _lines(rng, depth, N, count):
    ln = operand(rng, "p", (count, 4 * N + 1), depth)
    ln[count // 2], ln[count - 1] = (1 << depth) - 1, 0
    return ln


def _slots(rng, count, total, pitch):
    """`count` of `total` slots of `pitch` elements, shuffled, starting at element 1"""
    pick = rng.permutation(total)[:count]
    while np.all(np.diff(pick[:count // 2]) > 0) or np.all(np.diff(pick[count // 2:]) > 0):     # callers split it in two
        pick = rng.permutation(pick)
    return (1 + pick * pitch).astype(np.int32)


def intra_filter_case(depth, N, count, seed):
    rng = np.random.default_rng(seed)
    L = 4 * N + 1
    ln = _lines(rng, depth, N, count)
    ioff, ooff = _slots(rng, count, count + 3, L + 2), _slots(rng, count, count + 2, L + 3)
    src = operand(rng, "p", 2 + (count + 3) * (L + 2), depth)
    out = filled(GUARD_ROWS + (count + 2) * (L + 3), src.dtype)
    cells = np.zeros(out.shape, bool)
    for i in range(count):
        src[ioff[i]:ioff[i] + L] = ln[i]
        cells[ooff[i]:ooff[i] + L] = True
    bufs = {"in": src, "ioff": ioff, "out": out, "ooff": ooff}
    args = [depth, N, Buf("in"), Buf("ioff"), Buf("out"), Buf("ooff"), count, None]

    def job(o, i):
        return [("out", slice(ooff[i], ooff[i] + L), o.intra_filter(N, ln[i]))]
    return Case("x265hip_intra_filter_batch", "intra_filter", "N%d" % N, count, depth, bufs, ["out"], args, {"out": cells}, job=job, offsets=[(ioff, None), (ooff, None)])


def intra_allangs_case(depth, N, count, bLuma, seed):
    rng = np.random.default_rng(seed)
    L = 4 * N + 1
    o = Orc(depth)
    ln = _lines(rng, depth, N, count)
    filt = np.stack([o.intra_filter(N, ln[i]) for i in range(count)])
    off = _slots(rng, 2 * count, 2 * count + 5, L + 2)
    loff, foff = off[:count].copy(), off[count:].copy()
    src = operand(rng, "p", 2 + (2 * count + 5) * (L + 2), depth)
    for i in range(count):
        src[loff[i]:loff[i] + L], src[foff[i]:foff[i] + L] = ln[i], filt[i]
    out = filled((count + GUARD_ROWS, 33 * N * N), src.dtype)
    bufs = {"lines": src, "loff": loff, "foff": foff, "out": out}
    args = [depth, N, Buf("lines"), Buf("loff"), Buf("foff"), bLuma, Buf("out"), count, None]

    def job(o, i):
        return [("out", i, o.intra_allangs(N, ln[i], filt[i], bLuma).reshape(-1))]
    return Case("x265hip_intra_allangs_batch", "intra_allangs", "N%d bLuma%d" % (N, bLuma), count, depth, bufs, ["out"], args, {"out": dense_mask(out.shape, count)},
                job=job, offsets=[(loff, None), (foff, None)])


# ---- family 9: interpolation ------------------------------------------------------------------------------------------------------------------
CHROMA_SHAPES = [(2, 4), (4, 4), (6, 8), (8, 8), (12, 16), (16, 16), (32, 32)]
LUMA_SHAPES = [(8, 8), (16, 16), (64, 64), (12, 16), (32, 24), (4, 8), (48, 64)]          # the list of test_hip_parity.test_interp_batches


def interp_kinds(taps):
    """(kind, flags): every kind but HV at 4 taps, all seven at 8 taps; HPS also with the row extension"""
    return [(k, 0) for k in ("hpp", "hps", "vpp", "vps", "vsp", "vss")] + ([("hvpp", 0)] if taps == 8 else []) + [("hps", 1)]


def interp_case(kind, taps, depth, w, h, n, ext, seed, ny=24, nx=24):
    rng = np.random.default_rng(seed)
    short = kind in ("vsp", "vss")
    src = operand(rng, "a" if short else "p", (h + ny + 9, w + 2 * nx + 10), depth)
    ys, xs = src_origins(rng, n, ny, nx, y0=4, x0=5)
    rows = h + (taps - 1 if ext else 0)
    dy, dx, dshape = dst_grid(rng, n, w, rows, avoid=(src.shape[1],))
    D = filled(dshape, po.pix_dtype(depth) if kind in ("hpp", "vpp", "vsp", "hvpp") else np.int16)
    cx, cy = rng.integers(0, 8 if taps == 4 else 4, n), rng.integers(0, 4, n)
    cx[rng.integers(0, n)] = 0
    coeff = (cx | (cy << 4)) if kind == "hvpp" else cx
    bufs = {"src": src, "D": D, "oS": flat(ys, xs, src), "oD": flat(dy, dx, D), "coeff": coeff.astype(np.int32)}
    args = [IF_KINDS[kind], taps, depth, w, h, Buf("src"), src.shape[1], Buf("D"), D.shape[1], Buf("oS"), Buf("oD"), Buf("coeff"), 1 if ext else 0, n, None]

    def job(o, i):
        return [("D", (slice(dy[i], dy[i] + rows), slice(dx[i], dx[i] + w)), o.interp(kind, taps == 4, w, h, src, (int(ys[i]), int(xs[i])), int(cx[i]), int(cy[i]), ext))]
    c = Case("x265hip_interp_batch", "interp%d_%s%s" % (taps, kind, "_ext" if ext else ""), "%dx%d" % (w, h), n, depth, bufs, ["D"], args,
             {"D": block_mask(D.shape, dy, dx, rows, w)}, job=job, witness=lambda want: {"coeffIdx_0": bool((cx == 0).any())}, offsets=[(bufs["oS"], src.shape[1]), (bufs["oD"], D.shape[1])], pitches=[src.shape[1], D.shape[1]], width=w)
    return c


# ---- families 7 and 8: chroma edge filters, SAO edge offsets and statistics over a small picture ------------------------------------------------------
PIC_H, PIC_W = 136, 200            # the picture of test_hip_parity.test_loop_filter_primitives_match_oracle_and_golden
# x265hip_sao_job / x265hip_sao_stats_job of include/x265hip.h (the CPU tier checks them against the ctypes mirrors of x265_amd/hipprim.py)
SAO_JOB = np.dtype([("recOff", "<i8"), ("aux0", "<i8"), ("aux1", "<i8"), ("width", "<i4"), ("height", "<i4"), ("startX", "<i4"), ("offsets", "i1", 32),
                    ("signLeft", "i1", 2), ("reserved", "i1", 2)])
SAO_STATS_JOB = np.dtype([("diffOff", "<i8"), ("recOff", "<i8"), ("aux0", "<i8"), ("aux1", "<i8"), ("endX", "<i4"), ("endY", "<i4")])
SAO_REGION = 140                   # a job's part of the sign array: two buffers of up to 64 + 2 entries, 70 apart


def pel_filter_chroma_case(depth, edgeDir, n, seed):
    """Job i filters the four lines of its own 4x4 cell (the edge runs through its middle); all four maskP / maskQ combinations, tc 0 .. 24."""
    rng = np.random.default_rng(seed)
    ys, xs, shape = dst_grid(rng, n, 4, 4)
    plane = operand(rng, "p", shape, depth)
    S = shape[1]
    py, px = (ys, xs + 2) if edgeDir == 0 else (ys + 2, xs)
    tc = (rng.integers(0, 25, n) << (depth - 8)).astype(np.int32)
    combo = rng.permutation(n) % 4
    mP, mQ = (-(combo & 1)).astype(np.int32), (-(combo >> 1)).astype(np.int32)
    bufs = {"plane": plane, "off": (py * S + px).astype(np.int64), "tc": tc, "mP": mP, "mQ": mQ}
    step, offset = (S, 1) if edgeDir == 0 else (1, S)
    args = [depth, Buf("plane"), Buf("off"), step, offset, Buf("tc"), Buf("mP"), Buf("mQ"), n, None]
    cells = block_mask(shape, ys, xs + 1, 4, 2) if edgeDir == 0 else block_mask(shape, ys + 1, xs, 2, 4)

    def oracle():
        o, p = Orc(depth), plane
        for i in range(n):
            p = o.pel_filter_chroma(p, at(py, px, i), edgeDir, int(tc[i]), int(mP[i]), int(mQ[i]))
        return {"plane": p}

    def witness(want):
        return {"mask_combos": len(set(combo.tolist())), "filtered": bool((want["plane"] != plane).any())}
    c = Case("x265hip_pel_filter_chroma_batch", "pel_filter_chroma", "dir%d" % edgeDir, n, depth, bufs, ["plane"], args, {"plane": cells}, oracle=oracle, witness=witness,
             offsets=[(bufs["off"], None)])
    return c


def deblock_chroma_cases(depth, seed):
    """The chroma planes of the picture: every unit of every vertical edge of the 8-sample chroma grid in one launch, then every horizontal one on what that
    left — units in shuffled order, bs 0 / 1 / 2, per-unit QPs, a bypass array; the reference applies the units in the same order."""
    rng = np.random.default_rng(seed)
    H, W = PIC_H // 2, PIC_W // 2
    pmax = (1 << depth) - 1

    def blocky():
        b = np.kron(np.cumsum(rng.integers(-6, 7, size=(H // 4, W // 4)), axis=1) + 120, np.ones((4, 4), np.int64)) << (depth - 8)
        return np.clip(b + rng.integers(-1, 2, size=b.shape), 0, pmax).astype(po.pix_dtype(depth))
    cb, cr = blocky(), blocky()
    tcDiv2, cbOff, crOff = 1, 2, -3
    out = []
    for edgeDir in (0, 1):
        units = [(x, y) for y in range(0, H, 4) for x in range(8, W, 8)] if edgeDir == 0 else [(x, y) for y in range(8, H, 8) for x in range(0, W, 4)]
        units = [units[k] for k in rng.permutation(len(units))]
        n = len(units)
        bs = rng.integers(0, 3, n).astype(np.uint8)
        qpP, qpQ = rng.integers(18, 52, n).astype(np.int8), rng.integers(18, 52, n).astype(np.int8)
        byp = (rng.random((n, 2)) < 0.15).astype(np.uint8)
        xy = np.array(units, np.int32)
        bufs = {"cb": cb, "cr": cr, "xy": xy.reshape(-1), "bs": bs, "qpP": qpP, "qpQ": qpQ, "bypass": byp.reshape(-1)}
        args = [depth, Buf("cb"), Buf("cr"), W, edgeDir, Buf("xy"), Buf("bs"), Buf("qpP"), Buf("qpQ"), Buf("bypass"), tcDiv2, cbOff, crOff, n, None]
        ys, xs = xy[:, 1].astype(np.int64), xy[:, 0].astype(np.int64)
        cells = block_mask((H, W), ys, xs - 1, 4, 2) if edgeDir == 0 else block_mask((H, W), ys - 1, xs, 2, 4)

        def oracle(cb=cb, cr=cr, units=units, bs=bs, qpP=qpP, qpQ=qpQ, byp=byp, edgeDir=edgeDir, memo={}):
            if not memo:
                o = Orc(depth)
                fc = o._lf("orc_deblock_chroma_unit", [po.vp, po.vp, po.ip, po.ip] + [po.i32] * 10)
                b, r = cb.copy(), cr.copy()
                step, off = (W, 1) if edgeDir == 0 else (1, W)
                for i, (x, y) in enumerate(units):
                    fc(ptr(b, y, x), ptr(r, y, x), step, off, int(bs[i]), int(qpP[i]), int(qpQ[i]), 1, int(byp[i, 0]), int(byp[i, 1]), tcDiv2, cbOff, crOff, depth)
                memo.update(cb=b, cr=r)
            return dict(memo)
        def witness(want, cb=cb, cr=cr, bs=bs, byp=byp):
            return {"filtered": bool((want["cb"] != cb).any() and (want["cr"] != cr).any()), "skipped": bool((bs < 2).any()), "bypassed": bool(byp[bs == 2].any())}
        c = Case("x265hip_deblock_chroma_batch", "deblock_chroma", "dir%d" % edgeDir, n, depth, bufs, ["cb", "cr"], args, {"cb": cells, "cr": cells}, oracle=oracle,
                 offsets=[(xy[:, 1] * W + xy[:, 0], None)], guarded=False, witness=witness)
        want = c.oracle()
        out.append(c)
        cb, cr = want["cb"], want["cr"]
    return out


def sao_picture(rng, depth):
    """neighbouring samples often equal or one apart: every edge class occurs"""
    base = rng.integers(0, (1 << depth) - 8, size=(PIC_H // 4, PIC_W // 4))
    return (np.kron(base, np.ones((4, 4), np.int64)) + rng.integers(0, 3, size=(PIC_H, PIC_W))).astype(po.pix_dtype(depth))


def sao_ctus(rng):
    """(y, x, width, height) of the 64x64 CTUs of the picture inside a one-sample rim (ragged right and bottom ones), in shuffled order"""
    c = [(y, x, min(64, PIC_W - 1 - x), min(64, PIC_H - 1 - y)) for y in range(1, PIC_H - 1, 64) for x in range(1, PIC_W - 1, 64)]
    return [c[k] for k in shuffled(rng, rng.permutation(len(c)))]


def _sign_array(rng, n):
    """one SAO_REGION of signs per job at shuffled places, sentinels between and around them"""
    base = (3 + shuffled(rng, rng.permutation(n + 2)[:n]) * (SAO_REGION + 5)).astype(np.int64)
    aux = filled(3 + (n + 2) * (SAO_REGION + 5) + GUARD_ROWS, np.int8)
    cells = np.zeros(aux.shape, bool)
    for b in base:
        aux[b:b + SAO_REGION] = rng.integers(-1, 2, SAO_REGION)
        cells[b:b + SAO_REGION] = True
    return aux, base, cells


def sao_apply_case(depth, kind, seed):
    """kind 0 .. 4 = E0, E1, E1_2Rows, E2, E3: one job per CTU, each on one or two rows somewhere inside its CTU and one sample short of its width, so that
    no job reads what another writes (the entry's rule); every job its own offsets, signLeft and sign buffers."""
    rng = np.random.default_rng(seed)
    pic, cs = sao_picture(rng, depth), sao_ctus(rng)
    n, rows = len(cs), 2 if kind in (0, 2) else 1
    aux, base, acells = _sign_array(rng, n)
    jobs = np.zeros(n, SAO_JOB)
    pos = []
    for i, (y0, x0, cw, ch) in enumerate(cs):
        y = y0 + int(rng.integers(0, ch - rows))
        pos.append((y, x0))
        jobs[i]["recOff"], jobs[i]["width"], jobs[i]["height"] = y * PIC_W + x0, cw - 1, rows
        jobs[i]["offsets"][:5] = rng.integers(-7, 8, 5)
        jobs[i]["signLeft"] = rng.integers(-1, 2, 2)
        jobs[i]["startX"] = int(rng.integers(0, 2)) if kind == 4 else 0
        jobs[i]["aux0"], jobs[i]["aux1"] = base[i] + (1 if kind == 4 else 0), base[i] + 70
    cells = np.zeros(pic.shape, bool)
    for i, (y, x) in enumerate(pos):
        cells[y:y + rows, x + (int(jobs[i]["startX"]) + 1 if kind == 4 else 0):x + int(jobs[i]["width"])] = True
    bufs = {"plane": pic, "jobs": jobs}
    if kind:
        bufs["aux"] = aux
    args = [depth, kind, Buf("plane"), PIC_W, Buf("aux") if kind else None, Buf("jobs"), n, None]

    def oracle():
        o, p, a = Orc(depth), pic, aux.copy()
        for i in range(n):
            w, eo, b = int(jobs[i]["width"]), jobs[i]["offsets"][:5], int(base[i])
            if kind == 0:
                p = o.sao_e0(p, pos[i], eo, w, jobs[i]["signLeft"])
            elif kind in (1, 2):
                p, a[b:b + w] = o.sao_e1(p, pos[i], a[b:b + w], eo, w, rows)
            elif kind == 3:
                p, a[b:b + w + 1] = o.sao_e2(p, pos[i], a[b:b + w + 1], a[b + 70:b + 70 + w], eo, w)
            else:
                p, a[b:b + w + 1] = o.sao_e3(p, pos[i], a[b:b + w + 1], eo, int(jobs[i]["startX"]), w)
        return {"plane": p, "aux": a} if kind else {"plane": p}

    def witness(want):
        return {"changed": bool((want["plane"] != pic).any()), "signs_written": bool(kind == 0 or (want["aux"] != aux).any())}
    c = Case("x265hip_sao_apply_batch", "sao_apply", "kind%d" % kind, n, depth, bufs, ["plane", "aux"] if kind else ["plane"], args, {"plane": cells, "aux": acells},
             oracle=oracle, witness=witness, offsets=[(jobs["recOff"], None), (base, None)])
    return c


def sao_stats_case(depth, kind, seed):
    """kind 0 .. 4 = BO, E0, E1, E2, E3: every CTU of the picture in one launch; stats / count start non-zero and must end at start + the reference's sums."""
    rng = np.random.default_rng(seed)
    pic, cs = sao_picture(rng, depth), sao_ctus(rng)
    n, pmax, ncls = len(cs), (1 << depth) - 1, 32 if kind == 0 else 5
    aux, base, acells = _sign_array(rng, n)
    slot = shuffled(rng, rng.permutation(n))
    diff = rng.integers(-pmax, pmax + 1, size=(n, 64, 64)).astype(np.int16)          # diff[slot[i]] belongs to job i
    stats, count = filled((n + GUARD_ROWS, 32), np.int32), filled((n + GUARD_ROWS, 32), np.int32)
    stats[:n], count[:n] = rng.integers(-(1 << 20), 1 << 20, (n, 32)), rng.integers(1, 1 << 20, (n, 32))
    jobs = np.zeros(n, SAO_STATS_JOB)
    for i, (y0, x0, cw, ch) in enumerate(cs):
        jobs[i] = (int(slot[i]) * 4096, y0 * PIC_W + x0, base[i] + 1, base[i] + 71, cw, ch)
    bufs = {"diff": diff, "plane": pic, "jobs": jobs, "stats": stats, "count": count}
    if kind >= 2:
        bufs["aux"] = aux
    args = [depth, kind, Buf("diff"), Buf("plane"), PIC_W, Buf("aux") if kind >= 2 else None, Buf("jobs"), n, Buf("stats"), Buf("count"), None]

    def job(o, i):
        y0, x0, cw, ch = cs[i]
        b = int(base[i])
        st, ct, u1, ut = o.sao_stats(kind, diff[slot[i]], pic, (y0, x0), cw, ch, stats[i, :ncls], count[i, :ncls], aux[b:b + cw + 2], aux[b + 70:b + 72 + cw])
        res = [("stats", (i, slice(0, ncls)), st), ("count", (i, slice(0, ncls)), ct)]
        return res + ([("aux", slice(b, b + cw + 2), u1), ("aux", slice(b + 70, b + 72 + cw), ut)] if kind >= 2 else [])
    def witness(want):            # how many jobs counted a sample in each class
        return {"classes": (want["count"][:n, :ncls] > count[:n, :ncls]).sum(axis=0)}

    c = Case("x265hip_sao_stats_batch", "sao_stats", "kind%d" % kind, n, depth, bufs, ["stats", "count"] + (["aux"] if kind >= 2 else []), args,
             {"stats": dense_mask(stats.shape, n), "count": dense_mask(count.shape, n), "aux": acells}, job=job, witness=witness,
             offsets=[(jobs["recOff"], None), (jobs["diffOff"], None), (base, None)])
    return c


def loopfilter_cases(depth):
    for edgeDir in (0, 1):
        for n in NS:
            yield pel_filter_chroma_case(depth, edgeDir, n, _seed("pelc", depth, edgeDir, n))
    yield from deblock_chroma_cases(depth, _seed("dbc", depth))
    for kind in range(5):
        yield sao_apply_case(depth, kind, _seed("saoapply", depth, kind))
    for kind in range(5):
        yield sao_stats_case(depth, kind, _seed("saostats", depth, kind))


# ---- the tables: family -> (depths, promised launch count per depth, generator) -----------------------------------------------------------------------
def _seed(*parts):
    s = 0
    for p in parts:
        s = (s * 131 + (p if isinstance(p, int) else sum(ord(ch) * (k + 1) for k, ch in enumerate(p)))) % (1 << 31)
    return s


def ew_cases(depth):
    return (ew_case(e, depth, w, h, n, _seed("ew", e, depth, w, h, n)) for e in EW_ENTRIES for (w, h) in EW_SHAPES for n in NS)


def wave_cases(depth):
    for (w, h) in WAVE_SHAPES:
        for n in wave_counts(w, h):
            yield sse_case("sse_pp", depth, w, h, n, _seed("sse_pp", depth, w, h, n))
            for K in (3, 4):
                yield sad_xn_case(K, depth, w, h, n, _seed("sad", K, depth, w, h, n))


def wave16_cases(depth):
    for (w, h) in WAVE_SHAPES:
        for n in wave_counts(w, h):
            yield sse_case("sse_ss", None, w, h, n, _seed("sse_ss", w, h, n))
            yield sse_case("ssd_s", None, w, h, n, _seed("ssd_s", w, h, n))


DEQUANT_BRANCHES = [(2, 3), (8, 1)]     # (per, shift): shift + 4 > per rounds and shifts right; shift + 4 <= per clips and shifts left


def quant_cases(depth):
    for size in (4, 8, 16, 32):
        for n in NS:
            yield nquant_case(size, n, _seed("nquant", size, n))
            for per, shift in DEQUANT_BRANCHES:
                yield dequant_scaling_case(size, n, per, shift, _seed("dequant", size, n, per))
            yield denoise_case(size, n, _seed("denoise", size, n))


def dst4_cases(depth):
    return (dst4_case(depth, n, inv, _seed("dst4", depth, n, inv)) for n in NS for inv in (0, 1))


def smallops_cases(depth):
    for n in NS:
        for size in SQUARE:
            yield var_case(depth, size, n, _seed("var", depth, size, n))
            yield transpose_case(depth, size, n, _seed("transpose", depth, size, n))
        yield scale1d_case(depth, n, _seed("scale1d", depth, n))
        yield scale2d_case(depth, n, _seed("scale2d", depth, n))


INTRA_COUNTS = (7, 67)


def intra_cases(depth):
    for N in (4, 8, 16, 32):
        for count in INTRA_COUNTS:
            yield intra_filter_case(depth, N, count, _seed("filter", depth, N, count))
            for bLuma in (0, 1):
                yield intra_allangs_case(depth, N, count, bLuma, _seed("allangs", depth, N, count, bLuma))


def interp_cases(taps):
    def gen(depth):
        for (w, h) in (CHROMA_SHAPES if taps == 4 else LUMA_SHAPES):
            for kind, ext in interp_kinds(taps):
                for n in NS:
                    yield interp_case(kind, taps, depth, w, h, n, ext, _seed("interp", taps, kind, ext, depth, w, h, n))
    return gen


FAMILIES = {
    "elementwise": (DEPTHS, len(EW_ENTRIES) * len(EW_SHAPES) * len(NS), ew_cases),
    "wave_packed": (DEPTHS, len(WAVE_SHAPES) * 2 * 3, wave_cases),
    "wave_packed_int16": ((None,), len(WAVE_SHAPES) * 2 * 2, wave16_cases),
    "past_the_cap": ((8,), 3, lambda depth: iter(past_the_cap_cases())),
    "quant_denoise": ((None,), 4 * len(NS) * (2 + len(DEQUANT_BRANCHES)), quant_cases),
    "dst4": (DEPTHS, len(NS) * 2, dst4_cases),
    "smallops": (DEPTHS, len(NS) * (2 * len(SQUARE) + 2), smallops_cases),
    "intra": (DEPTHS, 4 * len(INTRA_COUNTS) * 3, intra_cases),
    "loopfilter": (DEPTHS, 2 * len(NS) + 2 + 5 + 5, loopfilter_cases),
    "interp4": (DEPTHS, len(CHROMA_SHAPES) * 7 * len(NS), interp_cases(4)),
    "interp8": (DEPTHS, len(LUMA_SHAPES) * 8 * len(NS), interp_cases(8)),
}
TABLES = [(f, d) for f, (depths, _, _) in FAMILIES.items() for d in depths]
