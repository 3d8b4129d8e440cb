"""CPU: what holds of any correct builder of the lane tables (csrc/batch_tables.hip), checked on the tables themselves.  The host
builders touch no HIP call, so tests/dropin/lane_tables_dump.cpp fills a TinyBatch by hand, builds the one-row, tile, coverage and
adaptive-rho tables and writes them next to the inputs they were built from.  The layout (LaneTab, VEC_*, ATAB_*) and the rule for
which entry lane j keeps for column k are restated here independently of csrc/lane_tables.hpp: the builders, the Riccati epilogue
and the sensitivity epilogue all go through that one mapping, so a transposed index in it fails here (profiles/lane_tables.md)."""
import os
import struct
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
KM = 4                                       # LIN_KMAX: the stride of the half-space blocks for up to 4 half-spaces per knot
VEC = dict(CB=0, CF=1, QR=2, SMASK=3, NIM=4, SOCFLAG=5, CONE_BASE=6, CONE_MU=7, RHO=8, LINFLAG=9, TLINFLAG=10)
ATAB = dict(AT=0, DK=256, DP=512, DC1=768, DC2=1024, DOUBLES=1280)
INPUTS = ("A B f Qw Rw Kinf Pinf Quu_inv AmBKt APf BPf dK dP dC1 dC2 x_min x_max u_min u_max Acx cx Acu cu "
          "Alin_x blin_x Alin_u blin_u tvA_x tvb_x tvA_u tvb_u").split()
GARGS = "mb mf1 mf2 pt cb cf qr lo hi sc ic ax bx au bu tax tbx tau tbu".split()
CASES = {(2, 2, 3): [], (6, 3, 10): ["cone=both", "ssoc=1", "isoc=1"], (20, 8, 10): []}
COMMON = ["bounds=xdiff", "lin=2", "sl=1", "il=1", "tlin=2", "tsl=1", "til=1"]


class Tab:
    """LaneTab{cols, lw}: four matrices [column][lane], 16 lane vectors, bounds [lo | hi][N][lw], the half-space blocks."""
    def __init__(self, cols, lw):
        self.cols, self.lw = cols, lw
        self.MB, self.MF1, self.MF2, self.PT, self.VEC = (i * cols * lw for i in range(5))
        self.BOUNDS = self.VEC + 16 * lw

    def lin_offset(self, N):
        return self.BOUNDS + 2 * N * self.lw

    def tlin_offset(self, N, km):
        return self.lin_offset(N) + 3 * km * self.lw

    def doubles(self, N, km):
        return self.tlin_offset(N, km) + 3 * N * km * self.lw

    def matrix(self, t, base):
        return t[base:base + self.cols * self.lw].reshape(self.cols, self.lw).T          # [lane j][column k]

    def vec(self, t, name):
        return t[self.VEC + VEC[name] * self.lw:][:self.lw]


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    exe = str(tmp_path_factory.mktemp("lane_tables") / "dump")
    csrc = os.path.join(ROOT, "tinympc_amd", "csrc")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-std=c++17", "-I", csrc, "-x", "hip", os.path.join(ROOT, "tests", "dropin", "lane_tables_dump.cpp"),
                    os.path.join(csrc, "batch_tables.hip"), "-o", exe], check=True, capture_output=True, timeout=600)
    cache = {}

    def run(shape, *keys):
        if (shape, keys) not in cache:
            out = exe + ".bin"
            subprocess.run([exe, "case", out] + [str(v) for v in shape] + list(keys), check=True, timeout=60)
            raw, at = open(out, "rb").read(), 0

            def vec():
                nonlocal at
                n = struct.unpack_from("i", raw, at)[0]
                v = np.frombuffer(raw, np.float64, n, at + 4)
                at += 4 + 8 * n
                return v
            r = {"tab": vec(), "ttab": vec(), "gtab": vec()}
            ints = struct.unpack_from("21i", raw, at)
            at += 84
            r["o"], r["uniform"] = dict(zip(GARGS, ints)), ints[19:]
            for name in INPUTS:
                r[name] = vec()
            r["atab"] = vec()
            assert at == len(raw)
            nx, nu = shape[:2]
            for name, rows, cols in (("A", nx, nx), ("B", nx, nu), ("Kinf", nu, nx), ("Pinf", nx, nx), ("Quu_inv", nu, nu), ("AmBKt", nx, nx),
                                     ("dK", nu, nx), ("dP", nx, nx), ("dC1", nu, nu), ("dC2", nx, nx)):
                if r[name].size:
                    r[name] = r[name].reshape(cols, rows).T                            # column-major
            cache[(shape, keys)] = r
        return cache[(shape, keys)]
    return run


def lane_tables(r, shape):
    """[(name, layout, table)] of the lane tables the shape has: the one-row layout only up to 16 rows."""
    nz = shape[0] + shape[1]
    out = [("tile", Tab(32, 16 if nz <= 16 else 32), r["ttab"])]
    return out + ([("one-row", Tab(16, 16), r["tab"])] if nz <= 16 else [])


@pytest.mark.parametrize("shape", list(CASES))
def test_matrix_and_vector_entries_are_the_problems_and_agree_across_tables(dump, shape):
    nx, nu, N = shape
    nz, ld = nx + nu, nx + nu + 1
    r = dump(shape, *COMMON, *CASES[shape])
    # what lane j keeps for column k, from the inputs alone ([j][k]; products summed in the builders' order, no FMA)
    mb, mf1, mf2, pt = (np.zeros((nz, nz)) for _ in range(4))
    mb[:nx, :nx], mb[:nx, nx:] = r["AmBKt"], -r["Kinf"].T
    mb[nx:, nx:] = r["Quu_inv"]
    for a in range(nu):
        for k in range(nx):
            s = 0.0
            for m in range(nu):
                s += r["Quu_inv"][a, m] * r["B"][k, m]
            mb[nx + a, k] = s
    mf1[:nx, :nx], mf1[nx:, :nx] = r["A"], -r["Kinf"]
    mf2[:nx, nx:] = r["B"]
    pt[:nx, :nx] = r["Pinf"].T
    cb = np.concatenate([r["APf"], [sum((r["Quu_inv"][a, m] * r["BPf"][m] for m in range(nu)), 0.0) for a in range(nu)]])
    cf = np.concatenate([r["f"], np.zeros(nu)])
    qr = np.concatenate([r["Qw"], r["Rw"]])
    g, o = r["gtab"], r["o"]
    for name, want in (("mb", mb), ("mf1", mf1), ("mf2", mf2), ("pt", pt)):
        got = g[o[name]:o[name] + nz * ld].reshape(nz, ld)
        assert np.array_equal(got[:, :nz], want) and not got[:, nz].any(), "coverage table " + name
    for name, want in (("cb", cb), ("cf", cf), ("qr", qr)):
        assert np.array_equal(g[o[name]:o[name] + nz], want), "coverage table " + name
    for label, T, t in lane_tables(r, shape):
        assert t.size == T.doubles(N, KM), label
        for base, want, name in ((T.MB, mb, "MB"), (T.MF1, mf1, "MF1"), (T.MF2, mf2, "MF2"), (T.PT, pt, "PT")):
            full = np.zeros((T.lw, T.cols))
            full[:nz, :nz] = want
            assert np.array_equal(T.matrix(t, base), full), "%s table %s[lane j][column k]" % (label, name)
        for name, want in (("CB", cb), ("CF", cf), ("QR", qr), ("SMASK", np.arange(nz) < nx), ("NIM", -1.0 * (np.arange(nz) >= nx)), ("RHO", np.zeros(nz))):
            full = np.zeros(T.lw)
            full[:nz] = want
            assert np.array_equal(T.vec(t, name), full), "%s table VEC_%s" % (label, name)


@pytest.mark.parametrize("shape", [s for s in CASES if s[0] + s[1] <= 16])
def test_w1_tile_table_holds_the_one_row_table(dump, shape):
    N = shape[2]
    r = dump(shape, *COMMON, *CASES[shape])
    R, T = Tab(16, 16), Tab(32, 16)
    for a, b in ((R.MB, T.MB), (R.MF1, T.MF1), (R.MF2, T.MF2), (R.PT, T.PT)):
        assert np.array_equal(r["ttab"][b:b + 256], r["tab"][a:a + 256]) and not r["ttab"][b + 256:b + 512].any()
    assert np.array_equal(r["ttab"][T.VEC:], r["tab"][R.VEC:], equal_nan=True)      # vectors, bounds, half-space blocks: same lw, same bytes
    assert r["ttab"].size - T.VEC == r["tab"].size - R.VEC == R.doubles(N, KM) - R.VEC


@pytest.mark.parametrize("shape", list(CASES))
def test_bounds_cones_and_half_spaces_sit_at_the_layouts_offsets(dump, shape):
    nx, nu, N = shape
    nz = nx + nu
    r = dump(shape, *COMMON, *CASES[shape])
    inf = np.inf
    for label, T, t in lane_tables(r, shape):
        lw = T.lw
        # bounds: state lanes knot i in slot i, input lanes knot i in slot i + 1 (slot 0 is a dummy), everything else (-inf, +inf)
        lo, hi = np.full((N, lw), -inf), np.full((N, lw), inf)
        lo[:, :nx], hi[:, :nx] = r["x_min"].reshape(N, nx), r["x_max"].reshape(N, nx)
        lo[1:, nx:nz], hi[1:, nx:nz] = r["u_min"].reshape(N - 1, nu), r["u_max"].reshape(N - 1, nu)
        assert np.array_equal(t[T.BOUNDS:T.BOUNDS + N * lw].reshape(N, lw), lo), label
        assert np.array_equal(t[T.BOUNDS + N * lw:T.lin_offset(N)].reshape(N, lw), hi), label
        # cones: flag per family, first lane and coefficient on the three lanes of every cone
        flag, base, mu = np.zeros(lw), np.full(lw, -1.0), np.zeros(lw)
        flag[:nx], flag[nx:nz] = float(r["Acx"].size > 0), float(r["Acu"].size > 0)
        for first, c, lane0 in ((r["Acx"], r["cx"], 0), (r["Acu"], r["cu"], nx)):
            for f, m in zip(first.astype(int), c):
                base[lane0 + f:lane0 + f + 3], mu[lane0 + f:lane0 + f + 3] = lane0 + f, m
        for name, want in (("SOCFLAG", flag), ("CONE_BASE", base), ("CONE_MU", mu)):
            assert np.array_equal(T.vec(t, name), want), "%s table VEC_%s" % (label, name)
        ones = np.zeros(lw)
        ones[:nz] = 1.0
        assert np.array_equal(T.vec(t, "LINFLAG"), ones) and np.array_equal(T.vec(t, "TLINFLAG"), ones), label
        # half-space blocks [coefficient | offset | squared norm][KM][lw]; blank: offset +inf, norm 1
        def block(rows_x, b_x, rows_u, b_u):
            blk = np.zeros((3, KM, lw))
            blk[1], blk[2] = inf, 1.0
            for rows, bs, lane0, n in ((rows_x, b_x, 0, nx), (rows_u, b_u, nx, nu)):
                for k, (row, bk) in enumerate(zip(rows, bs)):
                    nn = 0.0
                    for v in row:
                        nn += v * v
                    blk[0, k, lane0:lane0 + n], blk[1, k, lane0:lane0 + n], blk[2, k, lane0:lane0 + n] = row, bk, nn
            return blk.ravel()
        size = 3 * KM * lw
        assert np.array_equal(t[T.lin_offset(N):][:size], block(r["Alin_x"].reshape(2, nx), r["blin_x"], r["Alin_u"].reshape(1, nu), r["blin_u"])), label
        tax, tbx = r["tvA_x"].reshape(N, 2, nx), r["tvb_x"].reshape(N, 2)
        tau, tbu = r["tvA_u"].reshape(N - 1, 1, nu), r["tvb_u"].reshape(N - 1, 1)
        for s in range(N):                                                          # input lanes: slot s = knot s - 1
            want = block(tax[s], tbx[s], tau[s - 1] if s else [], tbu[s - 1] if s else [])
            assert np.array_equal(t[T.tlin_offset(N, KM) + s * size:][:size], want), "%s table, slot %d" % (label, s)
    assert tuple(r["uniform"]) == ((0, 0) if nz <= 16 else (-1, 0))                 # xdiff: one knot differs in a state bound


@pytest.mark.parametrize("shape", [s for s in CASES if s[0] + s[1] <= 16])
def test_adaptive_table_holds_what_the_atab_comments_state(dump, shape):
    nx, nu, _ = shape
    r = dump(shape, "prime=1")
    everything = np.concatenate([r[k].ravel() for k in ("A", "B", "dK", "dP", "dC1", "dC2")])
    assert np.unique(everything).size == everything.size                            # distinct primes: a transposition cannot hide
    want = np.zeros((5, 16, 16))                                                    # [table][column k][lane j]
    want[0, :nx, :nx], want[0, :nx, nx:nx + nu] = r["A"], r["B"]                    # ATAB_AT: A[k][j], B[k][j-nx]
    want[1, :nu, :nx], want[1, :nx, nx:nx + nu] = r["dK"], r["dK"].T                # ATAB_DK: dK[k][j] (state lanes), dK[j-nx][k] (input lanes)
    want[2, :nx, :nx] = r["dP"]                                                     # ATAB_DP: dP[k][j]
    want[3, :nu, :nu] = r["dC1"]                                                    # ATAB_DC1: dC1[k][j], lanes j < nu
    want[4, :nx, :nx] = r["dC2"]                                                    # ATAB_DC2: dC2[k][j]
    assert r["atab"].size == ATAB["DOUBLES"]
    for i, name in enumerate(("AT", "DK", "DP", "DC1", "DC2")):
        assert np.array_equal(r["atab"][ATAB[name]:ATAB[name] + 256].reshape(16, 16), want[i]), "ATAB_" + name


@pytest.mark.parametrize("shape,keys,want", [
    ((2, 2, 3), ("bounds=none",), 1),                       # never set: (-inf, +inf) at every knot
    ((2, 2, 3), ("bounds=same",), 1),
    ((20, 8, 10), ("bounds=same",), 1),
    ((6, 3, 10), ("bounds=xdiff",), 0),                     # one knot differs in a state bound
    ((6, 3, 10), ("bounds=udiff",), 0),                     # ... in an input bound
    ((6, 3, 10), ("bounds=xdiff", "sb=0"), 1),              # the differing family is switched off
    ((6, 3, 10), ("bounds=udiff", "ib=0"), 1),
    ((6, 3, 10), ("bounds=nan",), 0),                       # a NaN bound equals nothing, not even itself
    ((1, 1, 2), ("bounds=unan",), 0),                       # N = 2: the NaN sits in the only input knot
    ((1, 1, 2), ("bounds=same",), 1),
])
def test_the_uniform_flag_of_the_builders(dump, shape, keys, want):
    """box_is_uniform is the one place that decides whether the UB forms may run: both builders leave its verdict in the flag."""
    r = dump(shape, *keys)
    assert tuple(r["uniform"]) == ((want, want) if shape[0] + shape[1] <= 16 else (-1, want))
