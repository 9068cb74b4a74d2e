"""The GEMM cases of tests/test_gpu_gemm_variants.py, as data.

Kept apart from the GPU test so that tests/test_gemm_plan.py can ask the
planner (tns_gemm_plan, no GPU) which kernel each case reaches: the leaf census
there fails when a kernel instantiation is reached by no case here.

What each table variant supports is written here from the KIND column of
TNS_SHAPES (tensorium_amd/csrc/gemm_plan.hpp) and the large-NN forms' `applies`
comments; it is never asked of the library.
"""
import zlib
from dataclasses import dataclass, field, replace

import numpy as np

SENT = np.float32(-77.25)

# name, BM, BN, BK, MFMA edge, KIND — the tuning table in order
TILES = [
    ("128x128x32_w2x2", 128, 128, 32, 32, "full"),
    ("128x64x32_w2x2", 128, 64, 32, 32, "full"),
    ("64x128x32_w2x2", 64, 128, 32, 32, "full"),
    ("64x256x32_w1x4", 64, 256, 32, 32, "full"),
    ("32x256x32_w1x4", 32, 256, 32, 32, "full"),
    ("256x256x32_w2x4", 256, 256, 32, 32, "trans4"),
    ("64x64x32_w2x2", 64, 64, 32, 32, "full"),
    ("256x256x32_w2x2", 256, 256, 32, 32, "nn4"),
    ("256x256x16_w2x2", 256, 256, 16, 32, "nn4"),
    ("256x128x32_w2x2", 256, 128, 32, 32, "nn4"),
    ("128x256x32_w2x2", 128, 256, 32, 32, "nn4"),
    ("256x128x16_w2x2", 256, 128, 16, 32, "nn4"),
    ("64x64x32_w2x2_m16", 64, 64, 32, 16, "full"),
    ("32x32x32_w2x2_m16", 32, 32, 32, 16, "full"),
    ("64x32x32_w2x2_m16", 64, 32, 32, 16, "nn4"),
    ("32x64x32_w2x2_m16", 32, 64, 32, 16, "nn4"),
    ("128x128x32_w2x2_m16", 128, 128, 32, 16, "nn4"),
    ("256x256x32_w2x4_m16", 256, 256, 32, 16, "trans4"),
    ("128x64x32_w4x2", 128, 64, 32, 32, "nn4"),
    ("64x128x32_w2x4", 64, 128, 32, 32, "nn4"),
    ("128x128x32_w4x2", 128, 128, 32, 32, "nn4"),
    ("64x64x32_w2x2_d1", 64, 64, 32, 32, "nn4"),
    ("64x64x32_w2x4_m16", 64, 64, 32, 16, "nn4"),
]
# name, BM, BN, BK, 32-bit offsets — the large-NN forms (variant = len(TILES) + form)
NN_BIG = [
    ("256x256x32_w2x4_nn_big", 256, 256, 32, False),
    ("128x128x32_w2x2_nn_big", 128, 128, 32, False),
    ("256x128x32_w2x2_nn_big", 256, 128, 32, False),
    ("256x256x32_w4x4_nn_big", 256, 256, 32, False),
    ("256x128x16_w2x2_b2_nn_big", 256, 128, 16, False),
    ("256x256x32_w2x4_pp_nn_big", 256, 256, 32, False),
    ("256x256x32_w2x2_dma_nn_big", 256, 256, 32, True),
    ("256x256x32_w2x2_dma_flat_nn_big", 256, 256, 32, True),
    ("256x256x32_w2x2_dma_b32_nn_big", 256, 256, 32, True),
]
# the VALU chain variants (TNS_OPT_SDOT_FORM = 1 + v) and the residue-register
# forms (64 + v) of the sdot-order NT product
CHAINS = ["chains<nt64,r2,1x1,gm4>", "chains<nt128,r2,1x1,gm8>", "chains<nt256,r2,1x1,gm8>",
          "chains<nt64,r2,2x2,gm4>", "chains<nt256,r2,2x2,gm8>", "chains<nt128,r4,2x2,gm8>",
          "chains<nt256,r4,2x2,gm8>", "chains<nt256,r8,2x2,gm16>", "chains<nt256,r2,4x4,gm8>"]
RC = ["rc_64x64_w2x2_c8", "rc_64x64_w2x2x2_c4", "rc_64x32_w2x1x2_c4"]
VARIANT_NAMES = [t[0] for t in TILES] + [b[0] for b in NN_BIG]
TRANS = [(0, 0), (0, 1), (1, 0), (1, 1)]
TNAME = {(0, 0): "nn", (0, 1): "nt", (1, 0): "tn", (1, 1): "tt"}
ALPHA_BETA = [(1.0, 0.0), (0.5, 2.0), (1.0, 1.0), (-1.5, 0.25)]


@dataclass(frozen=True)
class Case:
    id: str
    ta: int
    tb: int
    M: int
    N: int
    K: int
    variant: int = -1
    lda: int = 0      # 0: the packed row length
    ldb: int = 0
    ldc: int = 0      # 0: N + 3
    offA: int = 0     # element offsets into the (256-byte aligned) buffers
    offB: int = 0
    offC: int = 5
    batch: int = 1
    strideA: int = -1  # -1: the packed image (rows * ld)
    strideB: int = -1
    strideC: int = -1  # -1: M * ldc + 7 (sentinels between the images)
    alpha: float = 1.0
    beta: float = 0.0
    strict: bool = True   # TNS_OPT_STRICT_BETA0
    nan_c: bool = False   # a NaN and an Inf in C0
    null_ab: bool = False  # K = 0: A and B passed as null
    nt_sdot: int = 1
    tt_exact: int = 1
    sdot_form: int = -1
    rows: tuple = ()      # sampled rows of C compared (empty: all of C)
    why: dict = field(default_factory=dict, compare=False)  # why an operand is scalar

    # ---- derived ---------------------------------------------------------------
    @property
    def rowsA(self):
        return self.K if self.ta else self.M

    @property
    def rowsB(self):
        return self.N if self.tb else self.K

    @property
    def extA(self):  # contiguous extent
        return self.M if self.ta else self.K

    @property
    def extB(self):
        return self.K if self.tb else self.N

    @property
    def LDA(self):
        return self.lda or max(1, self.extA)

    @property
    def LDB(self):
        return self.ldb or max(1, self.extB)

    @property
    def LDC(self):
        return self.ldc or self.N + 3

    @property
    def SA(self):
        return self.rowsA * self.LDA if self.strideA < 0 else self.strideA

    @property
    def SB(self):
        return self.rowsB * self.LDB if self.strideB < 0 else self.strideB

    @property
    def SC(self):
        return self.M * self.LDC + 7 if self.strideC < 0 else self.strideC

    @property
    def seed(self):
        return zlib.crc32(self.id.encode())

    @property
    def beta_mode(self):
        if self.beta == 1.0:
            return 1
        return 0 if self.beta == 0.0 and not self.strict else 2

    @property
    def forced_mfma(self):
        """Runs sgemm_kernel.hpp's tile (or a large-NN form): one ascending
        chain per element whatever the transposes."""
        return self.variant >= 0 or (self.tb and not self.ta and not self.nt_sdot) or \
            (self.tb and self.ta and not self.tt_exact)

    def vecA(self):
        return vec4(self.offA, self.LDA, self.SA, self.batch, self.extA)

    def vecB(self):
        return vec4(self.offB, self.LDB, self.SB, self.batch, self.extB)

    def plan_args(self):
        return dict(variant=self.variant, transA=self.ta, transB=self.tb, M=self.M, N=self.N,
                    K=self.K, lda=self.LDA, ldb=self.LDB, ldc=self.LDC, strideA=self.SA,
                    strideB=self.SB, strideC=self.SC, batch=self.batch,
                    alpha1=int(self.alpha == 1.0), beta_mode=self.beta_mode, epi=0,
                    a16=int(self.offA % 4 == 0), b16=int(self.offB % 4 == 0),
                    nt_sdot=self.nt_sdot, tt_exact=self.tt_exact, sdot_form=self.sdot_form)


def vec4(off, ld, stride, batch, extent):
    """An operand is staged by float4 (the four reasons it is not: the pointer,
    the leading dimension, the extent, the batch stride)."""
    return off % 4 == 0 and ld % 4 == 0 and extent % 4 == 0 and (batch <= 1 or stride % 4 == 0)


def supported(c: Case) -> bool:
    """The support table: KIND for the tiles, `applies` for the large-NN forms."""
    v = c.variant
    if v < 0:
        return True
    if v < len(TILES):
        kind = TILES[v][5]
        if kind == "full":
            return True
        both = c.vecA() and c.vecB()
        return both if kind == "trans4" else both and not c.ta and not c.tb
    _, bm, bn, bk, off32 = NN_BIG[v - len(TILES)]
    if c.ta or c.tb or c.M % bm or c.N % bn or c.K % bk:
        return False
    if c.LDA % 4 or c.LDB % 4 or c.offA % 4 or c.offB % 4:
        return False
    if c.batch > 1 and (c.SA % 4 or c.SB % 4):
        return False
    if off32 and (c.LDA * 32 > 0x7fffffff or (256 * c.LDC + c.N) * 4 > 0x7fffffff):
        return False
    return True


# ---- 1. the instantiation matrix ----------------------------------------------------
REASONS = ["ptr", "ld", "extent", "stride"]


def _pad4(x, mod=0):
    """The least value >= x that is `mod` modulo 4."""
    return x + (mod - x) % 4


def _with_scalar(c: Case, who: str, reason: str) -> Case:
    """c with operand `who` ('A' / 'B') kept off float4 staging for `reason`."""
    why = dict(c.why, **{who: reason})
    if reason == "ptr":
        return replace(c, why=why, **{"off" + who: 1})
    if reason == "ld":  # an odd leading dimension
        ld = (c.extA if who == "A" else c.extB) + 1
        return replace(c, why=why, **{"ld" + who.lower(): ld | 1})
    if reason == "extent":  # extent + 1 under a leading dimension that is a multiple of 4
        dim = ("M" if c.ta else "K") if who == "A" else ("K" if c.tb else "N")
        c = replace(c, why=why, **{dim: getattr(c, dim) + 1})
        return replace(c, **{"ld" + who.lower(): _pad4((c.extA if who == "A" else c.extB))})
    return replace(c, why=why, batch=2)  # (the strides: _fix_strides)


def _fix_strides(c: Case) -> Case:
    """Batch strides: 2 modulo 4 for an operand that is scalar by its stride,
    a multiple of 4 for every other."""
    if c.batch == 1:
        return c
    sa = _pad4(c.rowsA * c.LDA, 2 if c.why.get("A") == "stride" else 0)
    sb = _pad4(c.rowsB * c.LDB, 2 if c.why.get("B") == "stride" else 0)
    return replace(c, strideA=sa, strideB=sb)


def _alpha_beta(c: Case):
    """The four (alpha, beta) of the suite, the first with a NaN and an Inf in
    C0 under strict beta = 0, and the same NaN with strict mode off."""
    out = []
    for i, (al, be) in enumerate(ALPHA_BETA):
        out.append(replace(c, id=f"{c.id}/ab{i}", alpha=al, beta=be, nan_c=i == 0))
    out.append(replace(c, id=f"{c.id}/ab0-blas", alpha=1.0, beta=0.0, nan_c=True, strict=False))
    return out


def matrix_cases(v: int):
    """Every instantiation of table variant v: problem = two tiles per
    dimension, the second ragged, extents multiples of 4; K = two k-tiles and a
    tail."""
    name, bm, bn, bk, _, kind = TILES[v]
    out = []
    if kind == "full":
        for t, (ta, tb) in enumerate(TRANS):
            for w, (a4, b4) in enumerate([(1, 1), (1, 0), (0, 1), (0, 0)]):
                r, r2 = 1 + (v + t + w) % 7, 1 + (v + 2 * t + 3 * w) % 7
                c = Case(f"matrix/{name}/{TNAME[ta, tb]}/a{4 if a4 else 1}b{4 if b4 else 1}", ta,
                         tb, bm + 4 * r, bn + 4 * r2, 2 * bk + 8, variant=v)
                ra, rb = REASONS[(v + t) % 4], REASONS[(v + t + 1 + w) % 4]
                # NT: both contiguous extents are K, so K + 1 cannot make one alone scalar
                if (ta, tb) == (0, 1) and a4 != b4:
                    ra = "ptr" if ra == "extent" else ra
                    rb = "ld" if rb == "extent" else rb
                # TN / NN / TT: A's and B's extents are different dimensions
                if not a4:
                    c = _with_scalar(c, "A", ra)
                if not b4:
                    c = _with_scalar(c, "B", rb)
                c = _fix_strides(c)
                assert (c.vecA(), c.vecB()) == (bool(a4), bool(b4)), c
                out += _alpha_beta(c)
        return out
    if kind == "trans4":
        for t, (ta, tb) in enumerate(TRANS):
            c = Case(f"matrix/{name}/{TNAME[ta, tb]}/a4b4", ta, tb, bm + 4 * (1 + (v + t) % 7),
                     bn + 4 * (1 + (v + 3 * t) % 7), 2 * bk + 8, variant=v)
            out += _alpha_beta(c)
        out.append(_with_scalar(replace(c, id=f"matrix/{name}/refuse-scalar-A"), "A", "ptr"))
        return out
    c = Case(f"matrix/{name}/nn/a4b4", 0, 0, bm + 4 * (1 + v % 7), bn + 4 * (1 + v % 5), 2 * bk + 8,
             variant=v)
    out += _alpha_beta(c)
    out.append(replace(c, id=f"matrix/{name}/refuse-tn", ta=1))
    out.append(replace(c, id=f"matrix/{name}/refuse-nt", tb=1))
    out.append(_with_scalar(replace(c, id=f"matrix/{name}/refuse-scalar-A"), "A", REASONS[v % 3]))
    out.append(_fix_strides(_with_scalar(replace(c, id=f"matrix/{name}/refuse-scalar-B"), "B",
                                         REASONS[1 + v % 3])))
    return out


# ---- 2. K and edge sweep ----------------------------------------------------------------
def sweep_cases(v: int):
    name, bm, bn, bk, mf, kind = TILES[v]
    out = []
    for ta, tb in (TRANS if kind != "nn4" else [(0, 0)]) :
        for K in (0, 1, bk - 1, bk, bk + 1):
            for M, N in ((1, 1), (bm, bn), (bm + 1, bn + 1), (mf - 1, mf + 1)):
                c = Case(f"sweep/{name}/{TNAME[ta, tb]}/{M}x{N}x{K}", ta, tb, M, N, K, variant=v,
                         alpha=0.5, beta=2.0, null_ab=K == 0)
                if K == 0:  # leading dimensions a float4 kind accepts
                    c = replace(c, lda=_pad4(max(1, c.extA)), ldb=_pad4(max(1, c.extB)))
                out.append(c)
    return out


# ---- 3. batches ------------------------------------------------------------------------
def batch_cases(v: int):
    """batch = 3, A shared (strideA = 0), padded strides for B and C, an
    element offset on every operand (multiples of 4 where the variant needs
    float4 operands; odd ones too where it does not)."""
    out = []
    if v < len(TILES):
        name, bm, bn, bk, _, kind = TILES[v]
        M, N, K = bm + 4, bn + 8, bk + 8
        trans = [(0, 0)] if kind == "nn4" else [(0, 0), (1, 0)]
        offs = [(4, 8)] if kind != "full" else [(4, 8), (3, 1)]
    else:
        name, bm, bn, bk, _ = NN_BIG[v - len(TILES)]
        M, N, K, trans, offs = bm, bn, 64, [(0, 0)], [(4, 8)]
    for ta, tb in trans:
        for oa, ob in offs:
            c = Case(f"batch/{name}/{TNAME[ta, tb]}/off{oa}-{ob}", ta, tb, M, N, K, variant=v,
                     offA=oa, offB=ob, offC=5, batch=3, strideA=0, alpha=0.5, beta=2.0)
            out.append(replace(c, strideB=c.rowsB * c.LDB + 12))
    return out


# ---- 4. the MFMA kernel's NT / TT through the options -----------------------------------
def option_cases():
    """TNS_OPT_NT_SDOT = 0 / TNS_OPT_TT_EXACT = 0 at default dispatch, one shape
    per tile pick_tile_variant can return for tb = 1."""
    shapes = [("32x256x32_w1x4", 32, 300, 40, 1), ("64x256x32_w1x4", 64, 300, 40, 1),
              ("256x256x32_w2x4", 256, 256, 36, 240), ("64x128x32_w2x2", 65, 1024, 40, 1),
              ("128x64x32_w2x2", 65, 100, 40, 1)]
    out = []
    for tile, M, N, K, batch in shapes:
        for ta in (0, 1):
            c = Case(f"option/{'tt' if ta else 'nt'}/{tile}", ta, 1, M, N, K, batch=batch,
                     alpha=0.5, beta=2.0, nt_sdot=0, tt_exact=0)
            out.append((c, tile))
    return out


# ---- 5. one case per remaining plan leaf --------------------------------------------------
def _tile_rows(M, tile):
    """First and last row of the first, a middle and the last tile."""
    tiles = M // tile
    rows = []
    for t in sorted({0, tiles // 2, tiles - 1}):
        rows += [t * tile, t * tile + 1, t * tile + tile // 2, t * tile + tile - 1]
    return tuple(sorted(set(r for r in rows if r < M)))


def leaf_cases():
    """(case, leaf the planner must name), at default dispatch unless the leaf
    is reachable only when forced."""
    nb = len(TILES)
    out = []
    # the large-NN cascade: 4096 x 3072 is 192 tiles of 256 x 256
    big = dict(M=4096, N=3072, rows=_tile_rows(4096, 256))
    out += [
        (Case("leaf/nn_big/w4-rows-pre", 0, 0, K=256, **big), "nn_big/w4<alpha1=1,rows=1,pre=1>"),
        (Case("leaf/nn_big/w4-rows", 0, 0, K=128, alpha=0.5, beta=2.0, **big),
         "nn_big/w4<alpha1=0,rows=1,pre=0>"),
        (Case("leaf/nn_big/w4-flat", 0, 0, K=96, beta=1.0, **big),
         "nn_big/w4<alpha1=1,rows=0,pre=0>"),
        # w4 addresses a block's C rows in 32 bits: past that, the ping-pong form
        (Case("leaf/nn_big/pp", 0, 0, 256, 256, 64, batch=192, ldc=2097152, strideC=256,
              strideA=0, alpha=0.5, beta=2.0, rows=_tile_rows(256, 256)),
         "nn_big/256x256x32_w2x4_pp_nn_big"),
    ]
    # the remaining w4 instantiations and form 0: no shape picks them, forced
    for form, K, alpha, leaf in [(6, 256, 0.5, "alpha1=0,rows=1,pre=1"),
                                 (6, 128, 1.0, "alpha1=1,rows=1,pre=0"),
                                 (6, 64, 0.5, "alpha1=0,rows=0,pre=0"),
                                 (7, 64, 1.0, "alpha1=1,rows=0,pre=1"),
                                 (7, 256, 0.5, "alpha1=0,rows=0,pre=1"),
                                 (8, 256, 1.0, "alpha1=1,rows=1,pre=0")]:
        out.append((Case(f"leaf/nn_big/forced-{form}-k{K}-a{alpha}", 0, 0, 256, 512, K,
                         variant=nb + form, alpha=alpha, beta=2.0), f"nn_big/w4<{leaf}>"))
    out.append((Case("leaf/nn_big/forced-0", 0, 0, 256, 512, 96, variant=nb, alpha=0.5, beta=2.0),
                "nn_big/256x256x32_w2x4_nn_big"))
    # launch_sgemm_nt_sdot by shape
    nt = lambda cid, M, N, K, **kw: Case(f"leaf/nt_sdot/{cid}", 0, 1, M, N, K, alpha=0.5,
                                         beta=2.0, **kw)
    out += [
        (nt("chains1", 32, 27, 4100), "sdot_chains/chains<nt128,r2,1x1,gm8>/v4"),
        (nt("chains2", 64, 288, 4101), "sdot_chains/chains<nt256,r2,1x1,gm8>/v1"),
        (nt("chains6", 256, 250, 4096), "sdot_chains/chains<nt256,r4,2x2,gm8>/v4"),
        (nt("rc", 1000, 2100, 41), "sdot_rc/rc_64x64_w2x2x2_c4"),
        (nt("tn2-4", 1000, 2100, 1028, rows=_tile_rows(1000, 32)), "nt_sdot/tn<2,4,64>"),
        (nt("tn2-1-o32", 1000, 2100, 1029, rows=_tile_rows(1000, 32)), "nt_sdot/tn<2,1,64,o32>"),
        (nt("tn1-4-256", 288, 250, 16384, rows=_tile_rows(288, 32)), "nt_sdot/tn<1,4,256>"),
        (nt("tn1-1-256", 288, 250, 16385, rows=_tile_rows(288, 32)), "nt_sdot/tn<1,1,256>"),
        (nt("tn1-4", 45, 70, 36), "nt_sdot/tn<1,4,64>"),
        (nt("tn1-1", 45, 70, 37), "nt_sdot/tn<1,1,64>"),
    ]
    # every chains variant at both global-load widths, every residue-register form
    for v, name in enumerate(CHAINS):
        for K, w in ((1028, "v4"), (1029, "v1")):
            out.append((nt(f"forced-chains{v}-{w}", 17, 40, K, sdot_form=1 + v),
                        f"sdot_chains/{name}/{w}"))
    for v, name in enumerate(RC):
        out.append((nt(f"forced-rc{v}", 70, 90, 37, sdot_form=64 + v), f"sdot_rc/{name}"))
    # the tt kernel: 64 x 64 tiles, 128 x 128 from 512 of them
    out += [
        (Case("leaf/tt/r4", 1, 1, 70, 90, 37, alpha=0.5, beta=2.0), "tt/r4"),
        (Case("leaf/tt/r8", 1, 1, 130, 129, 19, batch=128, alpha=0.5, beta=2.0), "tt/r8"),
    ]
    return out


# the one leaf no case reaches: launch_tn<2,1,64> without 32-bit row offsets
# needs (M - 1) * lda + K > 2^31 - 1 elements in A or B: at least 8 GiB of
# operand and, at b64 >= 1024 tiles, as many rows to sum
EXEMPT = {"nt_sdot/tn<2,1,64>": "an operand past 2^31 elements (8 GiB)"}


def all_cases():
    """Every GPU case of tests/test_gpu_gemm_variants.py."""
    out = []
    for v in range(len(TILES)):
        out += matrix_cases(v) + sweep_cases(v)
    for v in range(len(VARIANT_NAMES)):
        out += batch_cases(v)
    out += [c for c, _ in option_cases()] + [c for c, _ in leaf_cases()]
    ids = [c.id for c in out]
    assert len(ids) == len(set(ids)), "duplicate case id"
    return out
