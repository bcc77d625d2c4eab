#!/usr/bin/env python3
"""Generator of the hand-scheduled FlashAttention-2 forward main block for D = 128 on gfx950.

Replaces the compiler-scheduled steady state of fa2_fwd_kernel.hip.h for the headline shape class
(reference counterpart: kernel_fp16.cu:381-508, the per-KV-block loop of fwd_kernel).  The output is
the body of ONE inline-asm statement (fa2_fwd_d128_{f16,bf16}.inc) that the HIP kernel
`fwd_asm_kernel` (fa2_fwd_d128.hip.h) wraps: the HIP side computes addresses, the asm block does
everything from the Q load to the normalised O tile staged in LDS, the HIP side stores it.

Shape of the computation (one workgroup = 4 waves = 256 Q rows, ONE wave per SIMD, 512 registers):
    wave w owns Q rows [64w, 64w+64) as two 32-row blocks qb = 0, 1; KV tiles of 64 rows.
    accumulator file:  O[qb][dt]  a[0:127]   (f32, 8 tiles of 32(d) x 32(q))
                       Q[qb][ks]  a[128:191] (MFMA B fragments, loaded once)
                       K[kvb][ks] a[192:255] (MFMA A fragments of the next tile, ds_read_b128 straight into AGPRs)
    arch VGPRs:        S/P banks  v[24:151]  (4 x 32: per q block two banks alternating by tile parity; P is packed IN PLACE)
                       V^T frags  v[152:215] (ds_read_b64_tr_b16)
    both products are "swapped" (S^T = K Q^T, O^T = V^T P^T) exactly as in fa2_fwd_kernel.hip.h, so a lane owns one
    Q row of each block and the softmax is lane-local plus one v_permlane32_swap.

Software pipeline.  Body B(t), t = -2 .. ntiles-1, is 64 MFMAs:
    MFMA  0..31  PV(t)        O[qb] += V(t)^T P(t)^T          (qb 0 then qb 1, four O accumulators per k-step)
    MFMA 32..63  QK(t+2)      S(t+2)[qb] = K(t+2) Q[qb]^T      (the four 32x32 S accumulators take turns)
  and between them ("gaps") the single-issue work, spread by the water-filling scheduler (Gen.place) so that the
  weighted issue load of every gap is the same:
    M0, M1  row max + rescale decision of tile t+1, q block 0 / 1     (gaps 2..9; tail bodies: masks first, gaps 2..23)
    E0, E1  exp / two row-sum chains / in-place pair packing of tile t+1   (gaps 10..63)
    K(t+2) fragment reads (gaps 0..15), V(t+1) transpose reads (gaps 33..39), the 8 LDS-DMA pieces of K(t+3), V(t+2) (gaps 10..27)
  One s_waitcnt + s_barrier per body.  The O rescale of the deferred-max scheme is a rare out-of-line block entered between
  the two MFMA phases (all of PV(t) is in O, nothing of tile t+1 yet), so every value at the old reference is scaled once.
Head / tail bodies are the same generator with streams switched off (and the tail masks switched on).

Persistent workgroups.  The HIP shell runs the statement once per (head, q block) item of the workgroup's list.  Bodies
ntwg-2 and ntwg-1 of an item stage the NEXT item's Q fragments and K(0), K(1), V(0) tiles (operands %22..%27; out-of-line
code entered from the guarded staging groups), and the next statement skips its load phase (flag bit 0).

Variants and developer options (Gen(..., opt=..., abl=..., trace=..., <window>=...), `--opt` on the command line; Gen.KEYS and
Gen.OPTS list every name, anything else is an error):
    opt=ct       folded scale (the fp16 bodies the library ships since 0.8; bf16 bodies: f32 scale): Q * scale*log2e rounded once to the I/O dtype
                 (pure_torch_ver.py:61); the running reference is the C operand of the first QK^T k-step (C tuples v[176:207],
                 V^T k-steps 2-3 in a[224:255], K fragments in a 32-register pool with counted lgkmcnt waits: sched.lds_waits);
                 opt=f32scale names the other body (the command line builds both anyway)
    opt=maxfirst the row-max stream in every body (no sum-check fast bodies)
    opt=qpre     the next item's Q fragments are prescaled inside the item's last body (measured, not shipped)
    m= e= vread= kread= kread_ct= dma= mmask= se0= se1= sc0= sc1=    gap windows a:b of the filler streams (d64_<name>: head dim 64 only)
    abl=...      timing-only ablations of the fast bodies (streams left out; results are wrong, cycle counts are not); needs --probe
    trace=1..10  s_memtime sums (phases / barrier / whole block / tail bodies) returned through the LSE outputs; needs --probe
Probes that were measured and then removed from the generator — the records stay under profiles/, DESIGN.md sections 3, 4 and 10 have the
numbers: syn= (synthetic fillers), stagger=, shift= (code placement), dmaw= (per-wave staging windows), vsplit=, w1=/w2= (scheduler
weights), opt=vagpr / expsep / chainpv / chainqk / nofma / noadd / ctk64 / ctc0 (profiles/r03_body_cycle_ablation.txt), opt=pkadd,
opt=nomix (profiles/r13_kbench_q_prescale_mix.txt), opt=lmfma (row sums on the matrix pipe of the 32x32 body:
profiles/r13_kbench_d64_sumcheck_ab.txt).
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.realpath(__file__)))
import gen_driver  # noqa: E402
import sched  # noqa: E402
from isa import A, S, V, Arg, Ins, Label, M0, Neg, OFF, Program, VCC, mk  # noqa: E402

THR = 8.0            # deferred rescale threshold, log2 units (FA2_DEFER_THR of the HIP kernel)
NEG_INF = float("-inf")
# "sum check" fast bodies (no row-max stream): a lane's partial row sum of one tile — formed anyway — bounds every P of that lane, so
# `tile sum <= PSUM_MAX` proves that no P overflows the 16-bit type it is rounded to (fp16: 65504) without looking at the scores
PSUM_MAX = 32768.0

# ---- inline-asm operands (order = the operand list of the asm statement in fa2_fwd_d128.hip.h)
A_LSE0, A_LSE1 = Arg(0), Arg(1)                    # "=&v" outputs: log2-domain LSE of this lane's row in q block 0 / 1
# Q goes global -> LDS by LDS-DMA like a K tile (whole rows per instruction, the K image's granule swizzle on the source side) into the wave's
# part of the epilogue image — idle until the item's epilogue — and from there into the fragment registers (ds_read_b128, the K fragment geometry):
# the 16 fragment loads of 16 bytes per lane from 32 different rows each that did this before cost ~250 cycles of issue apiece (profiles/r16_*)
A_QD0 = Arg(2)                                     # per-lane LDS-DMA source byte offset of piece 0 of a 16-row group of Q (row lane / G, swizzled granule)
A_QW = Arg(3, "s")                                 # byte offset of this wave's first Q row from the head base
A_QRS = Arg(4, "s", 4)                             # buffer descriptor of this head's Q matrix (rows >= Nq read as zeros)
A_KRS, A_VRS = Arg(5, "s", 4), Arg(6, "s", 4)      # buffer descriptors of this head's K / V matrix
A_KD0, A_VD0 = Arg(7), Arg(8)                      # per-lane LDS-DMA source byte offset (piece 0, tile 0), K / V
A_KR0, A_VR0 = Arg(9), Arg(10)                     # per-lane LDS read offset of K fragment k-step 0 / V^T fragment d-block 0
A_LIM0, A_LIM1 = Arg(11), Arg(12)                  # last-tile mask: kv index (local, minus 4*hi) must be <= this, per q block
A_C = Arg(13, "s")                                 # scale * log2(e), f32 bits
A_NTW, A_NTWG = Arg(14, "s"), Arg(15, "s")         # KV tiles of this wave / of the workgroup
A_KTILE, A_VTILE = Arg(16, "s"), Arg(17, "s")      # bytes between consecutive KV tiles in K / V
A_KROW4, A_VROW4 = Arg(18, "s"), Arg(19, "s")      # 4 * row bytes - 1024: source stride between the DMA pieces of a wave
A_LDSW = Arg(20, "s")                              # wave * 4096: this wave's quarter of a tile image
A_EPI = Arg(21)                                    # per-lane LDS byte address of the epilogue image: row l31, half hi
# persistent workgroups: the asm statement runs once per (head, q block) item of the workgroup's list; the last two bodies of
# an item stage the NEXT item's Q fragments and its K(0), K(1), V(0) tiles, and the next statement is told to skip its loads
A_FLAGS = Arg(22, "s")                             # bit 0: this item's Q / K(0) / K(1) / V(0) are already staged; bit 1: a next item exists; bit 2: ... with >= 2 KV tiles; bit 3: this item is a KV-split part
                                                   # bit 4: safe mode — no fast bodies (the redo of an item whose sum check met a non-finite P: see Gen.rare_sum)
                                                   # bit 5: the shell's own (sticky safe mode after a redo: it sets bit 4 with it); bits 8 .. 12, fwd_m16_gen.py only:
                                                   # the 16-byte granules a row really has when the head dim is below the body's (0: all — Gen16.trim_offsets)
A_NQW = Arg(23, "s")                               # the next item: byte offset of this wave's first Q row; Q / K / V descriptors
A_QT16 = Arg(24, "s")                              # 16 * Q row bytes: source stride between the 16-row groups of Q
A_NQRS = Arg(25, "s", 4)
A_NKRS, A_NVRS = Arg(26, "s", 4), Arg(27, "s", 4)
# KV-split parts (flag bit 3; fa2_fwd_ws): the item sweeps a KV range of its (head, q block) and leaves a normalised f32 partial tile in the
# caller's workspace instead of the 16-bit tile in LDS — float (((dt*4 + g) * 256 + row) * 8 + 4*hi + e) of the tile for d = 32dt + 8g + 4hi + e,
# the layout of the HIP kernels' parts (fa2_fwd_kernel.hip.h): a store instruction of the wave writes 1 KiB of consecutive bytes
A_WSB = Arg(28, "s", 2)                            # address of the part's tile
N_ARGS = 29

# ---- fixed registers (everything below is clobbered by the asm statement)
VBASE = 16


def SB(qb, par):                                   # S / P bank of q block qb, tile parity par: 32 VGPRs
    return V(VBASE + 64 * qb + 32 * par, 32)


def VF(dt, ks):                                    # V^T fragment (4 VGPRs)
    return V(144 + 16 * ks + 4 * dt, 4)


KR = [V(208 + i) for i in range(8)]                # K fragment read addresses, k-step ks
VR = [V(216 + i) for i in range(4)]                # V^T fragment read addresses, d block dt
KD = [V(220 + i) for i in range(4)]                # LDS-DMA source offsets of this wave's 4 pieces of a K tile
VD = [V(224 + i) for i in range(4)]
WSO = VD[2]                                        # part epilogue (the DMA offsets are dead by then): per-lane byte offset of row 64*wave + l31, half hi in the tile
LSUM = [V(228, 2), V(230, 2)]                      # running row sums, two chains (even / odd elements) per q block
LA = [LSUM[0][0], LSUM[1][0]]
LB = [LSUM[0][1], LSUM[1][1]]
FSC = [V(232), V(233)]                             # pending O rescale factor
MC = [V(234), V(235)]                              # reference max in log2 units (m * c)
TMP = [V(236 + i) for i in range(8)]               # scratch: row-max chains, rescale block, epilogue
EP_LT, EP_T, EP_INV = FSC[0], FSC[1], V(244)       # epilogue scratch (the softmax state above is dead by then)
DSH = [V(245), V(246)]                             # sum-check bodies: pending shift of the next tile's scores (see S_FIX)
RSCR = [V(248 + i) for i in range(4)]              # rare_sum: scratch of the O rescale (the other q block's TMP registers hold its live sum chains)
QD = [V(252 + i) for i in range(4)]                # LDS-DMA source offsets of the pieces of a 16-row group of Q (the seam reuses them as read addresses)

S_T, S_KOFF, S_VOFF, S_FLAG, S_TMP, S_TMP2 = S(60), S(61), S(62), S(63), S(64), S(65)
S_NFAST, S_D, S_WAVE = S(70), S(71), S(72)
S_NOVM, S_PF = S(66), S(67)                          # next item's loads are in flight (do not drain vmcnt) / this item came prefetched
S_FIX = S(68)                                        # sum-check bodies, folded scale: bit qb = the scores of the NEXT tile of q block qb were formed against the old reference (shift in DSH)
# staging of the NEXT item's Q into this wave's part of the epilogue image, one half of a 16-row group per body from t = 0 on (Gen.qstage_group):
S_QH = S(69)                                         # half groups staged so far (8 = all; also 8 when there is no next item); its parity is the body's
S_QM0, S_QSOFF, S_QSB = S(73), S(58), S(59)        # LDS address / source offset of the group being staged; LDS address of the wave's Q image
S_TA, S_TB, S_TC = S(74, 2), S(76, 2), S(78, 2)      # "trace" builds: s_memtime samples (body start, phase boundary, body end)
S_SUM = [S(80), S(81), S(82), S(83)]                 # cycle sums over the fast bodies: PV phase, QK phase, barrier, bodies
S_MARK = [S(86, 2), S(88, 2), S(90, 2), S(92, 2)]     # trace: block entry, first main body, epilogue start, block end
S_MARKH = [S(94, 2), S(96, 2)]                        # trace 5 / 6: past the entry barrier, past the first head body
S_MARKE = S(98, 2)                                    # trace 7: in front of the entry barrier (entry -> here = the wave's own entry work, here -> past the barrier = waiting for the others)
CLOBBER_S = list(range(58, 100))      # (s100 and above are reserved by the compiler on gfx950)




class Geo:
    """Head-dim dependent sizes of a forward body (HD = 128: the headline kernel; HD = 64: the reference harness's own shape and SDXL's)."""

    def __init__(self, hd):
        assert hd in (64, 128)
        self.HD = hd
        self.NKS = hd // 16                 # MFMA k-steps of Q.K^T
        self.NDT = hd // 32                 # 32-wide d blocks of O
        self.ROWB = 2 * hd                  # bytes per tile row
        self.SLOT_B = 64 * self.ROWB        # bytes of one K (or V) tile image
        self.NP = self.SLOT_B // 4096       # LDS-DMA pieces of 1 KiB per wave and tile
        self.RPP = 1024 // self.ROWB        # tile rows per piece
        self.K_SLOT, self.V_BASE = 0, 2 * self.SLOT_B
        self.EPI_ROWB = self.ROWB + 16      # bytes per staged O row (padded: conflict-free column writes and row reads)
        self.EPI_BASE = 4 * self.SLOT_B     # the epilogue image sits above the K / V rings: they hold the next item's first tiles by then
        self.FAIL_OFF = self.EPI_BASE + 4 * 64 * self.EPI_ROWB     # one word: a wave met a non-finite P in a sum-check body -> the shell redoes the item in safe mode
        self.LDS_BYTES = self.FAIL_OFF + 16
        self.QF0 = 32 * self.NDT            # accumulator file: O[qb][dt] | Q[qb][ks] | K[kvb][ks]
        self.KF0 = self.QF0 + 8 * self.NKS


G128 = Geo(128)
K_SLOT, V_BASE, SLOT_B = G128.K_SLOT, G128.V_BASE, G128.SLOT_B          # (module-level names: the HD = 128 geometry, used by the emulator harness)
EPI_ROWB, EPI_BASE, LDS_BYTES = G128.EPI_ROWB, G128.EPI_BASE, G128.LDS_BYTES   # 272, 65536, 135168


def OACC(qb, dt, g=G128):
    return A(16 * (g.NDT * qb + dt), 16)


def QF(qb, ks, g=G128):
    return A(g.QF0 + 4 * (g.NKS * qb + ks), 4)


def KF(kvb, ks, g=G128):
    return A(g.KF0 + 4 * (g.NKS * kvb + ks), 4)


def KF_POOL(kvb, ks):                              # "ct" kernels: a 32-register pool, k-step ks lives in slot ks % 4
    return A(192 + 8 * (ks % 4) + 4 * kvb, 4)


# "ct" kernels: the C operand of the first QK^T k-step = -(reference max), per q block.  An MFMA takes C and D from the same
# register file, so the tuples live in arch VGPRs — v[176:207], which the V^T fragments of k-steps 2, 3 vacate for a[224:255]
CT = [V(176, 16), V(192, 16)]


def VF_CT(dt, ks):
    return V(144 + 16 * ks + 4 * dt, 4) if ks < 2 else A(224 + 16 * (ks - 2) + 4 * dt, 4)


def VF64(dt, ks):                                  # head dim 64 with "ct": two d blocks per k-step, packed (v[144:175]) so that v[176:207] hold the C tuples
    return V(144 + 8 * ks + 4 * dt, 4)


class Gen:
    # Tunables of the schedule (gap windows [a, b) of the filler streams of a body), code-generation options, and
    # timing-only ablations ("abl": stream names left out of the FAST bodies — wrong results, tools/kbench.py prices the parts)
    # (windows: measured sweep in profiles/r02_window_sweep.txt — fragment reads early in their phase shorten the waits at the
    #  phase boundary and at the end of the body: 2664 -> 2580 cycles per body)
    DEFAULTS = {"m": (2.0, 10.0), "e": (10.0, 64.0), "vread": (33.0, 40.0), "kread": (0.0, 16.0), "dma": (10.0, 28.0),
                "mmask": (2.0, 24.0), "abl": (), "opt": (), "trace": (0.0, 0.0),
                "kread_ct": (16.0, 32.0),   # "ct" kernels: gap window of the K reads of k-steps 0..3 (4..7 follow their pool slots)
                # sum-check fast bodies (head dim 128): exp + row sums + check of q block 0 / 1, then the pair packing of q block 0 / 1.  Measured
                # (tools/kbench.py, one box, c2 / c4 TF; max-first bodies 1230 / 1245): check of q block 0 before MFMA 32 (no late shift for it)
                # 0:31 31:46 18:58 58:64 -> 1232 / 1251; 0:40 40:52 12:58 58:64 -> 1235 / 1251; 4:56 56:62 6:60 60:64 -> 1238 / 1256; these -> 1245 / 1264
                "se0": (0.0, 48.0), "se1": (8.0, 60.0), "sc0": (48.0, 58.0), "sc1": (60.0, 64.0)}

    # HD = 64: half the MFMAs per tile for the same softmax work, so the windows are those of a 32-gap body (16 PV-phase + 16 QK-phase MFMAs)
    DEFAULTS64 = {"m": (1.0, 6.0), "e": (6.0, 32.0), "vread": (17.0, 24.0), "kread": (0.0, 12.0), "dma": (3.0, 15.0), "mmask": (1.0, 14.0),
                  "se0": (0.0, 24.0), "se1": (4.0, 30.0), "sc0": (24.0, 29.0), "sc1": (30.0, 32.0)}

    # What the constructor and --opt accept (gen_driver.py): everything else is an error, not a silently built default body
    WINDOWS = ("m", "e", "vread", "kread", "kread_ct", "dma", "mmask", "se0", "se1", "sc0", "sc1")
    KEYS = ("abl", "opt", "trace") + WINDOWS + tuple("d64_" + w for w in WINDOWS)
    OPTS = ("ct", "f32scale", "maxfirst", "qpre")
    # ... and what emits bodies that are WRONG BY DESIGN (timing probes) or that only exist for measurements: needs --probe
    PROBE_KEYS, PROBE_OPTS = ("abl", "trace"), ()
    STEM = "fa2d128"                  # labels of the inline-asm statement: .Lfa2d128_<name>_%=

    def __init__(self, bf16=False, hd=128, **cfg):
        assert not gen_driver.unknown(type(self), cfg), gen_driver.unknown(type(self), cfg)
        self.g = Geo(hd)
        self.cfg = dict(self.DEFAULTS)
        if hd == 64:
            self.cfg.update(self.DEFAULTS64)
        for k, v in cfg.items():          # "d64_<key>": a schedule tunable of the head-dim-64 body only (window sweeps, tools/kbench.py)
            if k.startswith("d64_"):
                if hd == 64:
                    self.cfg[k[4:]] = v
            else:
                self.cfg[k] = v
        self.opt = set(self.cfg["opt"])
        self.ct = "ct" in self.opt        # folded scale: Q * c rounded once, -m enters the first QK^T k-step as its C operand (no extra MFMAs)
        self.fold = self.ct               # prescaled Q, S leaves the MFMA as (score - reference)
        # opt=qpre (measured, not shipped: profiles/r16_kbench_eq2_tail_prescale_ab.txt, +-0.3 %): the NEXT item's Q fragments are prescaled between the
        # MFMAs of the item's last body instead of at the next statement's entry — 1.8 k stall cycles less per item and no wall time: the chip is
        # power-limited, a launch takes what its ENERGY takes, and a stall costs none
        self.qpre = self.fold and "qpre" in self.opt
        g = self.g
        # head dim 128 + "ct": the C tuples take v[176:207], so V^T k-steps 2-3 move to a[224:255] and the K fragments shrink to a 32-register pool;
        # head dim 64 has the room (half the V^T fragments, half the accumulator file): only the V^T fragments are packed
        self.pool = self.ct and hd == 128
        self.kf = KF_POOL if self.pool else (lambda kvb, ks: KF(kvb, ks, g))
        self.vf = (VF_CT if hd == 128 else VF64) if self.ct else VF
        self.qf = lambda qb, ks: QF(qb, ks, g)
        self.oacc = lambda qb, dt: OACC(qb, dt, g)
        # "sum check" fast bodies (the default; opt=maxfirst keeps the row-max stream everywhere): see stream_exp_sum.  The 64 v_add_f32 of the row
        # sums double as the overflow check and replace the 44-instruction row-max stream (row sums on the matrix pipe of this 32 x 32 body lost
        # against them: profiles/r13_kbench_d64_sumcheck_ab.txt)
        self.sumchk = "maxfirst" not in self.opt
        self.lm = False                   # (fwd_m16_gen.py, opt=lm: row sums on the matrix pipe AND fast bodies without a row-max stream)
        self.check_gaps = {}              # (body name, q block) -> the gap its sum check landed in
        self.npv = 8 * g.NDT              # MFMAs of the PV phase (both q blocks) ...
        self.nqk = 4 * g.NKS              # ... and of the QK phase
        self.ng = self.npv + self.nqk     # MFMAs (= gaps) per body
        self.bf16 = bf16
        self.mfma = "v_mfma_f32_32x32x16_bf16" if bf16 else "v_mfma_f32_32x32x16_f16"
        self.cvt = "v_cvt_pk_bf16_f32" if bf16 else "v_cvt_pk_f16_f32"
        self.p = Program()
        self.rare = []            # out-of-line blocks appended after the main code

    # ------------------------------------------------------------------ MFMA lists
    def pv_mfmas(self, par, qb):
        out = []
        for ks in range(4):
            pfrag = SB(qb, par).sub(16 * (ks >> 1) + 8 * (ks & 1), 4)
            for dt in range(self.g.NDT):
                out.append(mk(self.mfma, self.oacc(qb, dt), self.vf(dt, ks), pfrag, self.oacc(qb, dt), tag="mfma"))
        return out

    def qk_mfmas(self, par):
        """S(t+2) for both q blocks; the four 32x32 accumulators take turns (a dependent MFMA is four issues away)."""
        out = []
        for ks in range(self.g.NKS):
            for qb in range(2):
                for kvb in range(2):
                    dst = SB(qb, par).sub(16 * kvb, 16)
                    c0 = CT[qb] if self.ct else 0
                    out.append(mk(self.mfma, dst, self.kf(kvb, ks), self.qf(qb, ks), c0 if ks == 0 else dst, tag="mfma"))
        return out

    # ------------------------------------------------------------------ filler streams
    def stream_exp(self, qb, par):
        """P = 2^(S*c - m*c) in place (folded-scale kernels: P = 2^S, the MFMA delivered S = x - m), two row-sum chains,
        pairs packed in place; skewed by pair so that consecutive instructions of the stream are independent."""
        b = SB(qb, par)
        out = []
        for k in range(16 + 3):
            F, E, Ad, C = [], [], [], []
            if k < 16 and not self.fold:                      # stage 0: x = s*c - m*c
                e = 2 * k
                F.append(mk("v_fma_f32", b[e], b[e], A_C, Neg(MC[qb]), tag="valu"))
                F.append(mk("v_fma_f32", b[e + 1], b[e + 1], A_C, Neg(MC[qb]), tag="valu"))
            if 0 <= k - 1 < 16:                               # stage 1: 2^x
                e = 2 * (k - 1)
                E.append(mk("v_exp_f32", b[e], b[e], tag="trans"))
                E.append(mk("v_exp_f32", b[e + 1], b[e + 1], tag="trans"))
            if 0 <= k - 2 < 16:                               # stage 2: row sums
                e = 2 * (k - 2)
                Ad.append(mk("v_add_f32", LA[qb], LA[qb], b[e], tag="valu"))
                Ad.append(mk("v_add_f32", LB[qb], LB[qb], b[e + 1], tag="valu"))
            if 0 <= k - 3 < 16:                               # stage 3: pack the pair in place
                e = 2 * (k - 3)
                C.append(mk(self.cvt, b[8 * (e // 8) + (e % 8) // 2], b[e], b[e + 1], tag="valu"))
            out += F + E + Ad + C
        return out

    def stream_exp_sum(self, qb, par):
        """Fast bodies without a row-max stream.  P = 2^(S*c - m*c) against the CURRENT reference m (folded-scale kernels: P = 2^S) for the whole
        q block, the two row-sum chains started afresh for the tile (TA, TB), the tile sums added to the running sums — and ONE check: this lane's
        partial row sum of the tile, TA + TB, bounds each of its 32 P from above, so `TA + TB <= PSUM_MAX` (2^15) proves that every P fits the
        16-bit type it is about to be rounded to (fp16 overflows at 65504) and that none is inf / NaN — the reference may then stay where it is:
        rounding is relative, a P of 2^15 is as exact as a P of 1, O and l are f32.  The 16 v_max3 + exchange + decision of the max-first bodies
        (stream_max: ~22 instructions per q block and tile) become 3; the reference moves, out of line (rare_sum), only when the check fails.
        The pair packing (stream_pack) follows the check: the rare block needs the unpacked f32 P."""
        b = SB(qb, par)
        ta, tb, ts = TMP[4 * qb], TMP[4 * qb + 1], TMP[4 * qb + 2]
        out = []
        for k in range(16 + 2):
            F, E, Ad = [], [], []
            if k < 16 and not self.fold:                       # stage 0: x = s*c - m*c
                e = 2 * k
                F.append(mk("v_fma_f32", b[e], b[e], A_C, Neg(MC[qb]), tag="valu"))
                F.append(mk("v_fma_f32", b[e + 1], b[e + 1], A_C, Neg(MC[qb]), tag="valu"))
            if 0 <= k - 1 < 16:                               # stage 1: 2^x
                e = 2 * (k - 1)
                E.append(mk("v_exp_f32", b[e], b[e], tag="trans"))
                E.append(mk("v_exp_f32", b[e + 1], b[e + 1], tag="trans"))
            if 1 <= k - 2 < 16:                               # stage 2: the tile's two sum chains (pair 0 enters with pair 1)
                e = 2 * (k - 2)
                if k - 2 == 1:
                    Ad.append(mk("v_add_f32", ta, b[0], b[2], tag="valu"))
                    Ad.append(mk("v_add_f32", tb, b[1], b[3], tag="valu"))
                else:
                    Ad.append(mk("v_add_f32", ta, ta, b[e], tag="valu"))
                    Ad.append(mk("v_add_f32", tb, tb, b[e + 1], tag="valu"))
            out += F + E + Ad
        out.append(mk("v_add_f32", LA[qb], LA[qb], ta, tag="valu"))
        out.append(mk("v_add_f32", LB[qb], LB[qb], tb, tag="valu"))
        out.append(mk("v_add_f32", ts, ta, tb, tag="valu"))
        lab = self.p.fresh("rare_s")
        # not (limit >= sum): also true for a NaN sum (the literal has to be src0 of a VOPC).  (a list inside a stream is an atomic group: the branch and its return label stay together)
        out.append([mk("s_nop", 0, tag="salu"), mk("v_cmp_nge_f32", VCC, PSUM_MAX, ts, tag="valu"),
                    mk("s_cbranch_vccnz", Label(lab), tag="branch"), Ins("label", (Label(lab + "_ret"),))])
        self.pending_rare_sum.append((lab, qb, par))
        return out

    def stream_pack(self, qb, par):
        b = SB(qb, par)
        return [mk(self.cvt, b[8 * (e // 8) + (e % 8) // 2], b[e], b[e + 1], tag="valu") for e in range(0, 32, 2)]

    def rare_sum(self, lab, qb, par, fix):
        """Out of line, sum-check bodies: a lane's tile sum of q block qb exceeded PSUM_MAX.  All 32 f32 P of the tile are still unpacked in the bank:
        the row maximum of P (both lane halves) gives the growth d = max(0, ceil(log2 max P)) of the reference, and everything at the old reference —
        this tile's P, the running sums (this tile's share included), the O accumulators (all of PV(t) of this q block was issued gaps ago) — is
        multiplied by 2^-d, an exact power of two.  Folded-scale kernels also rewrite the C tuple of the coming QK^T products; `fix`: the first k-step
        of the NEXT tile's QK^T has been issued with the old tuple already, so those scores get the shift at the start of the next body (S_FIX, DSH).
        A maximum at or beyond 2^120 (a score 120+ log2 units above the reference: P at, or past, the edge of f32 — or a NaN input) is not repaired here:
        the wave raises the workgroup's flag word in LDS and goes on; the shell runs the item again in safe mode (A_FLAGS bit 4: max-first bodies only)."""
        b = SB(qb, par)
        mxa, mxb, t, t2 = TMP[4 * qb], TMP[4 * qb + 1], TMP[4 * qb + 2], TMP[4 * qb + 3]
        g = self.g
        r = [Ins("label", (Label(lab),))]
        r.append(mk("v_mov_b32", t2, t))                            # t = TMP[4qb+2] is the tile sum the check read: it carries an inf / NaN the maximum may drop
        for (mx, off) in ((mxa, 0), (mxb, 16)):                     # (mxa, mxb: the tile's sum chains, already added to the running sums)
            r.append(mk("v_max3_f32", mx, b[off], b[off + 1], b[off + 2]))
        for i in range(6):
            for (mx, off) in ((mxa, 0), (mxb, 16)):
                r.append(mk("v_max3_f32", mx, mx, b[off + 3 + 2 * i], b[off + 4 + 2 * i]))
        r.append(mk("v_max3_f32", mxa, mxa, b[15], b[31]))
        r.append(mk("v_max_f32", mxa, mxa, mxb))
        r.append(mk("v_mov_b32", t, mxa))
        r.append(mk("s_nop", 1))
        r.append(mk("v_permlane32_swap_b32", mxa, t))
        r.append(mk("v_max_f32", mxa, mxa, t))                      # row maximum of P
        r.append(mk("s_nop", 0))
        r.append(mk("v_add_f32", t2, t2, mxa))
        fail = lab + "_fail"
        r.append(mk("s_nop", 0))
        # not (2^120 > tile sum + row maximum): inf or NaN in some lane — or a growth close to 2^7 octaves: the factor 2^-d must stay a NORMAL f32
        # (v_exp_f32 flushes denormal results to zero: 2^-127, 2^-128 would wipe the row — found on the GPU by rows whose maximum sat in (2^126, 2^128))
        r.append(mk("v_cmp_ngt_f32", VCC, float(2.0 ** 120), t2))
        r.append(mk("s_cbranch_vccnz", Label(fail)))
        r.append(mk("v_log_f32", t, mxa))
        r.append(mk("s_nop", 0))
        r.append(mk("v_max_f32", t, 0, t))                          # rows that stayed below their reference keep it (d = 0)
        r.append(mk("s_nop", 0))
        r.append(mk("v_ceil_f32", t, t))                            # d: a whole number of octaves -> every factor below is an exact power of two
        r.append(mk("s_nop", 0))
        r.append(mk("v_exp_f32", t2, Neg(t)))                       # 2^-d
        r.append(mk("v_add_f32", MC[qb], MC[qb], t))                # the reference moves up by d
        r.append(mk("s_nop", 0))
        for e in range(32):
            r.append(mk("v_mul_f32", b[e], b[e], t2))
        r.append(mk("v_mul_f32", LA[qb], LA[qb], t2))
        r.append(mk("v_mul_f32", LB[qb], LB[qb], t2))
        if self.ct:
            r.append(mk("v_sub_f32", mxb, 0, MC[qb]))
            r.append(mk("s_nop", 0))
            for i in range(16):
                r.append(mk("v_mov_b32", CT[qb][i], mxb))
            if fix:
                r.append(mk("v_mov_b32", DSH[qb], t))
                r.append(mk("s_or_b32", S_FIX, S_FIX, 1 << qb))
        # O[qb] *= 2^-d (the MFMAs of PV(t) on these accumulators were issued at least a dozen gaps ago; the nops cover the last one's latency)
        r.append(mk("s_nop", 15))
        r.append(mk("s_nop", 15))
        for dt in range(g.NDT):
            acc = self.oacc(qb, dt)
            for i in range(0, 16, 4):
                for j in range(4):
                    r.append(mk("v_accvgpr_read_b32", RSCR[j], acc[i + j]))
                r.append(mk("s_nop", 1))
                for j in range(4):
                    r.append(mk("v_mul_f32", RSCR[j], RSCR[j], t2))
                r.append(mk("s_nop", 1))
                for j in range(4):
                    r.append(mk("v_accvgpr_write_b32", acc[i + j], RSCR[j]))
        r.append(mk("s_nop", 7))
        r.append(mk("s_branch", Label(lab + "_ret")))
        r.append(Ins("label", (Label(fail),)))
        r.append(mk("v_mov_b32", t, S_WAVE))                         # this wave's own flag word (four words: no two waves write the same bytes)
        r.append(mk("v_mov_b32", t2, 1))
        r.append(mk("v_lshlrev_b32", t, 2, t))
        r.append(mk("s_nop", 0))
        r.append(mk("v_add_u32", t, g.FAIL_OFF, t))
        r.append(mk("s_nop", 0))
        r.append(mk("ds_write_b32", t, t2))
        r.append(mk("s_waitcnt", lgkmcnt=0))
        r.append(mk("s_branch", Label(lab + "_ret")))
        return r

    def rare_fix(self, lab, par):
        """Out of line, start of a body (folded-scale sum-check kernels): q blocks flagged in S_FIX had their reference moved after the first QK^T
        k-step of THIS body's softmax tile had been issued with the old C tuple: shift those scores by the pending amount."""
        r = [Ins("label", (Label(lab),))]
        r.append(mk("s_nop", 15))                  # the QK^T MFMAs that wrote the bank ended the previous body
        r.append(mk("s_nop", 15))
        for qb in range(2):
            skip = self.p.fresh("fix_skip")
            r.append(mk("s_bitcmp1_b32", S_FIX, qb))
            r.append(mk("s_cbranch_scc0", Label(skip)))
            b = SB(qb, par)
            for e in range(32):
                r.append(mk("v_sub_f32", b[e], b[e], DSH[qb]))
            r.append(Ins("label", (Label(skip),)))
        r.append(mk("s_mov_b32", S_FIX, 0))
        r.append(mk("s_nop", 1))
        r.append(mk("s_branch", Label(lab + "_ret")))
        return r

    def stream_max(self, qb, par, masked, first=False):
        """mask (tail bodies) -> row max of the 32 scores of this lane -> half-wave exchange -> rescale decision."""
        b = SB(qb, par)
        out = []
        lim = A_LIM0 if qb == 0 else A_LIM1
        mxa, mxb, t, t2 = TMP[4 * qb], TMP[4 * qb + 1], TMP[4 * qb + 2], TMP[4 * qb + 3]
        if masked:
            # element r of kv half kvb is kv_local = 32*kvb + (r&3) + 8*(r>>2) (4*hi is folded into lim): kept iff <= lim
            out.append(mk("v_mov_b32", t2, NEG_INF, tag="valu"))      # (a literal next to vcc would need two constant-bus reads)
            for kvb in range(2):
                for r in range(16):
                    kvl = 32 * kvb + (r & 3) + 8 * (r >> 2)
                    out.append([mk("v_cmp_le_i32", VCC, kvl, lim, tag="valu"),
                                mk("v_cndmask_b32", b[16 * kvb + r], t2, b[16 * kvb + r], VCC, tag="valu")])
        for (mx, off) in ((mxa, 0), (mxb, 16)):
            out.append(mk("v_max3_f32", mx, b[off], b[off + 1], b[off + 2], tag="valu"))
        for i in range(6):
            for (mx, off) in ((mxa, 0), (mxb, 16)):
                out.append(mk("v_max3_f32", mx, mx, b[off + 3 + 2 * i], b[off + 4 + 2 * i], tag="valu"))
        out.append(mk("v_max3_f32", mxa, mxa, b[15], b[31], tag="valu"))
        out.append(mk("v_max_f32", mxa, mxa, mxb, tag="valu"))
        out.append(mk("v_mov_b32", t, mxa, tag="valu"))
        out.append([mk("s_nop", 1, tag="salu"), mk("v_permlane32_swap_b32", mxa, t, tag="valu")])
        out.append(mk("v_max_f32", mxa, mxa, t, tag="valu"))
        lab = self.p.fresh("rare_m")
        # (a list inside a stream is an atomic group: the scheduler keeps it contiguous — here a branch and its return label)
        if self.fold:
            # S already is (score - reference) in log2 units: its row max IS the growth.  Tile 0 adopts its own maximum
            # whatever the sign (the reference starts at 0, not at -inf: it travels through the MFMA as 16-bit terms).
            if first:
                out.append([mk("s_branch", Label(lab), tag="branch"), Ins("label", (Label(lab + "_ret"),))])
            else:
                out.append([mk("s_nop", 0, tag="salu"), mk("v_cmp_lt_f32", VCC, THR, mxa, tag="valu"),
                            mk("s_cbranch_vccnz", Label(lab), tag="branch"), Ins("label", (Label(lab + "_ret"),))])
            self.rare.append(self.rare_m_ct(lab, qb, b, mxa, mxb, t, t2, first))
            return out
        out.append(mk("v_fma_f32", t2, mxa, A_C, Neg(MC[qb]), tag="valu"))
        out.append([mk("v_cmp_lt_f32", VCC, THR, t2, tag="valu"), mk("s_cbranch_vccnz", Label(lab), tag="branch"),
                    Ins("label", (Label(lab + "_ret"),))])
        # out-of-line: move the reference (kept in scaled units m*c), scale the row sums now, leave the O rescale pending
        r = [Ins("label", (Label(lab),))]
        r.append(mk("v_mul_f32", t, A_C, mxa))                          # tile max * c
        r.append(mk("s_nop", 0))
        r.append(mk("v_max_f32", t, t, MC[qb]))                         # new reference
        r.append(mk("s_nop", 0))
        r.append(mk("v_sub_f32", mxb, MC[qb], t))                       # (m_old - m_new) * c  (<= 0; -inf on the first tile)
        r.append(mk("s_nop", 0))
        r.append(mk("v_exp_f32", mxb, mxb))
        r.append(mk("v_mov_b32", MC[qb], t))
        if not first:               # the q block's first tile: O is still all zeros, nothing to rescale later
            r.append(mk("s_or_b32", S_FLAG, S_FLAG, 1 << qb))
        r.append(mk("s_nop", 0))
        r.append(mk("v_mul_f32", LA[qb], LA[qb], mxb))
        r.append(mk("v_mul_f32", LB[qb], LB[qb], mxb))
        r.append(mk("v_mov_b32", FSC[qb], mxb))
        r.append(mk("s_branch", Label(lab + "_ret")))
        self.rare.append(r)
        return out

    def rare_m_ct(self, lab, qb, b, mxa, mxb, t, t2, first):
        """"ct" kernels, out of line: the reference of q block qb moves by d = max(row max, 0) (tile 0: = row max).  The C tuple
        of the next QK^T is rewritten with the new -reference, the scores of THIS tile — formed against the old reference — are
        shifted by the difference actually applied, the row sums are scaled now and the O rescale is left pending."""
        r = [Ins("label", (Label(lab),))]
        if not first:
            r.append(mk("v_max_f32", mxa, 0, mxa))                      # rows that did not grow keep their reference
            r.append(mk("s_nop", 0))
        r.append(mk("v_add_f32", mxb, MC[qb], mxa))                     # new reference
        r.append(mk("s_nop", 0))
        r.append(mk("v_sub_f32", t, mxb, MC[qb]))                       # the shift as applied
        r.append(mk("v_sub_f32", mxa, 0, mxb))                          # -reference for the C tuple
        r.append(mk("v_mov_b32", MC[qb], mxb))
        r.append(mk("s_nop", 0))
        for e in range(32):
            r.append(mk("v_sub_f32", b[e], b[e], t))                    # this tile's scores, now against the new reference
        for i in range(16):
            r.append(mk("v_mov_b32", CT[qb][i], mxa))
        r.append(mk("v_exp_f32", t2, Neg(t)))                           # factor for everything accumulated at the old one
        if not first:
            r.append(mk("s_or_b32", S_FLAG, S_FLAG, 1 << qb))
        r.append(mk("s_nop", 0))
        r.append(mk("v_mul_f32", LA[qb], LA[qb], t2))
        r.append(mk("v_mul_f32", LB[qb], LB[qb], t2))
        r.append(mk("v_mov_b32", FSC[qb], t2))
        r.append(mk("s_nop", 1))
        r.append(mk("s_branch", Label(lab + "_ret")))
        return r

    def stream_kread(self, par):
        out = []
        g = self.g
        for ks in range(g.NKS):
            for kvb in range(2):
                out.append(mk("ds_read_b128", self.kf(kvb, ks), KR[ks], tag="lds", offset=g.K_SLOT + par * g.SLOT_B + kvb * 32 * g.ROWB))
        return out

    def stream_vread(self, par):
        out = []
        g = self.g
        for ks in range(4):
            for dt in range(g.NDT):
                off = g.V_BASE + par * g.SLOT_B + 16 * ks * g.ROWB
                out.append(mk("ds_read_b64_tr_b16", self.vf(dt, ks).sub(0, 2), VR[dt], tag="lds", offset=off))
                out.append(mk("ds_read_b64_tr_b16", self.vf(dt, ks).sub(2, 2), VR[dt], tag="lds", offset=off + 8 * g.ROWB))
        return out

    def dma_group(self, which, slot_par, guarded, ahead):
        """The 4 LDS-DMA pieces of this wave's quarter of one K or V tile (tile index = t + ahead): image bytes
        [wave*4096 + i*1024, +1024), i.e. tile rows 16*wave + 4*i + lane/16.  M0 holds the quarter's LDS address, the piece
        is selected by the instruction offset (which also advances the source address: KD / VD are biased by -1024*i).
        Guarded bodies (everything but the fast loop): past this item's last tile, the K group of body ntwg-2 stages the
        NEXT item's K(0), K(1) and Q fragments and the V group of body ntwg-1 its V(0) (out of line; both rings and the Q
        registers are idle by then), and the end-of-body wait stops draining vmcnt."""
        out = []
        rs, vd, soff = (A_KRS, KD, S_KOFF) if which == "k" else (A_VRS, VD, S_VOFF)
        g = self.g
        base = (g.K_SLOT if which == "k" else g.V_BASE) + slot_par * g.SLOT_B
        skip = None
        if guarded:
            skip = self.p.fresh("dma_skip")
            nxt = self.p.fresh("dma_next")
            out.append(mk("s_add_u32", S_TMP2, S_T, ahead, tag="salu"))
            out.append(mk("s_cmp_lt_i32", S_TMP2, A_NTWG, tag="salu"))
            out.append(mk("s_cbranch_scc0", Label(nxt), tag="branch"))
            r = [Ins("label", (Label(nxt),))]
            r.append(mk("s_bitcmp1_b32", A_FLAGS, 1))
            r.append(mk("s_cbranch_scc0", Label(skip)))
            r.append(mk("s_sub_u32", S_TMP2, S_TMP2, 1))          # K: t + 2, V: t + 1 ...
            r.append(mk("s_cmp_eq_u32", S_TMP2, A_NTWG))         # ... == ntwg: body ntwg-2 (K) / ntwg-1 (V)
            r.append(mk("s_cbranch_scc0", Label(skip)))
            r.append(mk("s_mov_b32", S_NOVM, 1))
            nrs = A_NKRS if which == "k" else A_NVRS
            nbase = g.K_SLOT if which == "k" else g.V_BASE
            r.append(mk("s_add_u32", M0, A_LDSW, nbase))
            r.append(mk("s_nop", 0))
            for i in range(g.NP):
                r.append(mk("buffer_load_dwordx4", vd[i], nrs, 0, offen=True, offset=1024 * i, lds=True))
            if which == "k":
                one = self.p.fresh("dma_next_one")
                r.append(mk("s_bitcmp1_b32", A_FLAGS, 2))        # the next item has a second tile (causal items differ in length)
                r.append(mk("s_cbranch_scc0", Label(one)))
                r.append(mk("s_add_u32", M0, A_LDSW, g.K_SLOT + g.SLOT_B))
                r.append(mk("s_nop", 0))
                for i in range(g.NP):
                    r.append(mk("buffer_load_dwordx4", vd[i], nrs, A_KTILE, offen=True, offset=1024 * i, lds=True))
                r.append(Ins("label", (Label(one),)))
                r += self.seam_q_reads()
            r.append(mk("s_branch", Label(skip)))
            if which == "k":
                # groups of Q the bodies so far did not stage (a short item, a wave that left the fast loop early): now, AHEAD of the K tiles, so that one
                # counted wait below covers them
                at = [i for i, x in enumerate(r) if x.op == "s_mov_b32" and x.ops[0] is S_NOVM][0] + 1
                r[at:at] = self.seam_q_rest()
            self.rare.append(r)
        out.append([mk("s_add_u32", M0, A_LDSW, base, tag="salu"), mk("s_nop", 0, tag="salu")])
        for i in range(g.NP):
            out.append(mk("buffer_load_dwordx4", vd[i], rs, soff, tag="dma", offen=True, offset=1024 * i, lds=True))
        if guarded:
            out.append(Ins("label", (Label(skip),)))
            flat = []
            for x in out:
                flat.extend(x if isinstance(x, list) else [x])
            return [flat]         # one atomic group: the guard's SCC and branch must not be interleaved with other streams
        return out

    # ------------------------------------------------------------------ the next item's Q through LDS
    def q_group_loads(self, rs, soff, half=None):
        """LDS-DMA pieces of ONE 16-row group of Q (M0 = LDS address of the group, soff = its source offset): all NP, or half 0 / 1 of them."""
        g = self.g
        idx = range(g.NP) if half is None else range(half * g.NP // 2, (half + 1) * g.NP // 2)
        return [mk("buffer_load_dwordx4", QD[i], rs, soff, tag="dma", offen=True, offset=1024 * i, lds=True) for i in idx]

    def qstage_group(self, par):
        """Bodies t >= 0 of an item stage the NEXT item's Q: half a 16-row group per body (body parity = half), 8 bodies for the wave's 64 rows.
        S_QH counts the halves (its parity is the body's: every body from t = 0 on carries this group); 8 = done, or nothing to stage."""
        g = self.g
        skip = self.p.fresh("qst_skip")
        out = [mk("s_cmp_lt_u32", S_QH, 8, tag="salu"), mk("s_cbranch_scc0", Label(skip), tag="branch"),
               mk("s_mov_b32", M0, S_QM0, tag="salu"), mk("s_add_u32", S_QH, S_QH, 1, tag="salu")]
        out += self.q_group_loads(A_NQRS, S_QSOFF, half=par)
        if par == 1:
            out.append(mk("s_add_u32", S_QM0, S_QM0, g.NP * 1024, tag="salu"))
            out.append(mk("s_add_u32", S_QSOFF, S_QSOFF, A_QT16, tag="salu"))
        out.append(Ins("label", (Label(skip),)))
        return [out]          # one atomic group

    def q_prescale_reg(self, src, qreg, t0, t1):
        """Folded scale: one register of Q fragments (two 16-bit values) * scale*log2(e), rounded ONCE to the I/O dtype — the reference oracle's
        contract `scale * q_frags` (pure_torch_ver.py:61) — from src into the fragment register qreg, an AGPR (t0, t1: scratch)."""
        r = []
        if not self.bf16:
            # fp16: each half straight through the mixed-precision fma — f16 x f32 scale, rounded once to f16 into its half of the word
            r.append(mk("v_fma_mixlo_f16", t0, src, A_C, 0, tag="valu", op_sel="[0,0,0]", op_sel_hi="[1,0,0]"))
            r.append(mk("v_fma_mixhi_f16", t0, src, A_C, 0, tag="valu", op_sel="[1,0,0]", op_sel_hi="[1,0,0]"))
            r.append(mk("s_nop", 0, tag="salu"))
            r.append(mk("v_accvgpr_write_b32", qreg, t0, tag="valu"))
            return r
        r.append(mk("v_lshlrev_b32", t0, 16, src, tag="valu"))
        r.append(mk("v_and_b32", t1, 0xffff0000, src, tag="valu"))
        r.append(mk("v_mul_f32", t0, A_C, t0, tag="valu"))
        r.append(mk("v_mul_f32", t1, A_C, t1, tag="valu"))
        r.append(mk("s_nop", 0, tag="salu"))
        r.append(mk(self.cvt, t0, t0, t1, tag="valu"))
        r.append(mk("s_nop", 0, tag="salu"))
        r.append(mk("v_accvgpr_write_b32", qreg, t0, tag="valu"))
        return r

    def stream_qprescale(self):
        """Folded-scale kernels, the body at t = ntwg - 1 of an item that has a successor (TC / ST variants `q`): the NEXT item's raw Q fragments — read
        from the staged image at the seam, one body earlier — are prescaled in place between this body's MFMAs, so the next statement's entry finds
        them final (1.8 k cycles of bare VALU work per item before: profiles/r16_*).  One atomic group per register, four scratch pairs in rotation."""
        g = self.g
        out = []
        for i in range(8 * g.NKS):
            qreg = self.qf(i // (4 * g.NKS), (i % (4 * g.NKS)) // 4)[i % 4]
            t0, t1 = TMP[2 * (i & 3)], TMP[2 * (i & 3) + 1]
            src = DSH[i & 1] if self.bf16 else t1      # (the bf16 form reads src after writing t0: it gets a register of its own)
            grp = [mk("v_accvgpr_read_b32", src, qreg, tag="valu"), mk("s_nop", 0, tag="salu")]
            out.append(grp + self.q_prescale_reg(src, qreg, t0, t1))
        return out

    def qpre_check(self, target):
        """-> target when this is the item's last body (t = ntwg - 1) and a next item exists: its Q fragments were read at the seam, one body ago."""
        p = self.p
        no = p.fresh("qpre_no")
        p.emit("s_add_u32", S_TMP2, S_T, 1)
        p.emit("s_cmp_eq_u32", S_TMP2, A_NTWG)
        p.emit("s_cbranch_scc0", Label(no))
        p.emit("s_bitcmp1_b32", A_FLAGS, 1)
        p.emit("s_cbranch_scc1", Label(target))
        p.label(no)

    def seam_q_rest(self):
        """Seam (body ntwg - 2, out of line): 16-row groups of the next item's Q that are not fully staged yet are staged whole (a half-staged group is
        staged again: same bytes)."""
        g = self.g
        r = []
        for j in range(4):
            sk = self.p.fresh("qrest_skip")
            r.append(mk("s_cmp_ge_u32", S_QH, 2 * j + 2))
            r.append(mk("s_cbranch_scc1", Label(sk)))
            r.append(mk("s_add_u32", M0, S_QSB, j * g.NP * 1024))
            r.append(mk("s_mov_b32", S_TMP, A_NQW))
            for _ in range(j):
                r.append(mk("s_add_u32", S_TMP, S_TMP, A_QT16))
            r += self.q_group_loads(A_NQRS, S_TMP)
            r.append(Ins("label", (Label(sk),)))
        r.append(mk("s_mov_b32", S_QH, 8))
        return r

    def seam_q_reads(self):
        """... and the fragments are read into the (idle) Q registers: everything older than the K tiles just issued has landed after one counted wait.
        The read addresses are the K fragment ones moved to the wave's Q image; they take the DMA offset registers (dead: S_QH = 8)."""
        g = self.g
        r = []
        two, waited = self.p.fresh("qrd_two"), self.p.fresh("qrd_waited")
        r.append(mk("s_bitcmp1_b32", A_FLAGS, 2))
        r.append(mk("s_cbranch_scc1", Label(two)))
        r.append(mk("s_waitcnt", vmcnt=g.NP))
        r.append(mk("s_branch", Label(waited)))
        r.append(Ins("label", (Label(two),)))
        r.append(mk("s_waitcnt", vmcnt=2 * g.NP))
        r.append(Ins("label", (Label(waited),)))
        for k0 in range(0, g.NKS, 4):
            for i in range(4):
                r.append(mk("v_add_u32", QD[i], S_QSB, KR[k0 + i]))
            r.append(mk("s_nop", 0))
            for qb in range(2):
                for i in range(4):
                    r.append(mk("ds_read_b128", self.qf(qb, k0 + i), QD[i], offset=qb * 32 * g.ROWB))
            if k0 + 4 < g.NKS:
                r.append(mk("s_nop", 0))
        return r

    # ------------------------------------------------------------------ scheduler (shared with the backward generator: sched.py)
    place = staticmethod(sched.place)

    def place_pool_kreads(self, load, slots, par):
        """32-register fragment pool: k-steps 0..3 are read during the PV phase, k-step ks >= 4 goes into the slot of ks - 4
        as soon as the four MFMAs of that k-step are issued (12 MFMAs ahead of its own first use)"""
        cfg = self.cfg
        kr = self.stream_kread(par)
        self.place(load, slots, kr[:8], cfg["kread_ct"][0], cfg["kread_ct"][1], 3)
        for ks in range(4, 8):
            g = 32 + 4 * (ks - 4) + 3
            for kvb in range(2):
                it = kr[2 * ks + kvb]
                load[g] += sched.weight(it)
                slots[g].append((g + 0.5 + 0.1 * kvb, 3, it))

    def ct_reader_gaps(self, qb):
        """(first, last) gap of the MFMAs that read the C tuple(s) of q block qb: the first Q.K^T k-step of the NEXT tile."""
        return self.npv + 2 * qb, self.npv + 2 * qb + 1

    def qk_phase(self, par, s1, s2, fast):
        """the MFMAs of a body's second phase (fwd_m16_gen.py adds the row-sum links of its lm bodies)"""
        return self.qk_mfmas(par) if s2 else [None] * self.nqk

    def body_end(self, par, name, fast, s1):
        """hook: behind a body's last gap, ahead of its book-keeping and barrier (fwd_m16_gen.py: the row-sum check of the lm fast bodies)"""

    # ------------------------------------------------------------------ one body
    def body(self, par, pv=True, s1=True, s2=True, masked=False, guarded=True, name="body", first=False, dma=True, qpre=False):
        """B(t) with t & 1 == par.  pv: PV(t); s1: softmax of tile t+1 (M0, M1, E0, E1) and the V(t+1) reads; s2: K(t+2)
        reads and QK(t+2).  masked: tile t+1 is this wave's last one (causal diagonal / ragged tail masks); first: tile
        t+1 is tile 0.  Appends to self.p."""
        p = self.p
        cfg = self.cfg
        fast = name.startswith("F")
        abl = set(cfg["abl"]) if fast else set()
        ng = self.ng
        mf = []
        mf += self.pv_mfmas(par, 0) if pv else [None] * (self.npv // 2)
        mf += self.pv_mfmas(par, 1) if pv else [None] * (self.npv // 2)
        mf += self.qk_phase(par, s1, s2, fast)
        if "mfma" in abl:
            mf = [None] * ng
        trace = fast and 0 < cfg["trace"][0] < 9
        # trace 9 / 10: cycles of the tail bodies by kind (TA, TB | TC, ST), barrier included
        tkind = {"TA": 0, "TB": 1, "TC": 2, "ST": 3}.get(name[:2]) if cfg["trace"][0] in (9.0, 10.0) else None
        if trace or tkind is not None:
            p.emit("s_memtime", S_TA)
        if not pv:
            # no PV MFMAs separate this body's first VALU reads of S from the QK^T MFMAs that ended the previous body
            p.emit("s_nop", 15)
            p.emit("s_nop", 15)
        load = [0.0] * ng
        slots = [[] for _ in range(ng)]
        # fast bodies of the sum-check kernels carry no row-max stream (stream_exp_sum); head / tail / guarded bodies keep it — they also are the
        # whole sweep of an item that is redone in safe mode
        sumchk = self.sumchk and fast and s1 and not masked and not first and not abl
        self.pending_rare_sum = []
        if s1 and self.sumchk and self.ct and not first and not self.lm:
            # scores formed against a reference that moved after their first k-step was issued (rare_sum, `fix`) get their shift before anything reads them
            lab = p.fresh("rare_f")
            p.emit("s_cmp_lg_u32", S_FIX, 0)
            p.emit("s_cbranch_scc1", Label(lab))
            p.label(lab + "_ret")
            self.rare.append(self.rare_fix(lab, par ^ 1))
        if s1 and sumchk:
            self.place(load, slots, self.stream_exp_sum(0, par ^ 1), cfg["se0"][0], cfg["se0"][1], 0)
        elif s1:
            mw = cfg["mmask"] if masked else cfg["m"]
            ew = (mw[1], cfg["e"][1])
            if "max" not in abl:
                self.place(load, slots, self.stream_max(0, par ^ 1, masked, first), mw[0], mw[1], 0)
                self.place(load, slots, self.stream_max(1, par ^ 1, masked, first), mw[0], mw[1], 1)
        if dma and "dma" not in abl:
            grp = self.dma_group("k", par ^ 1, guarded, 3) + self.dma_group("v", par, guarded, 2)
            if not name.startswith("H"):
                # t >= 0: every such body carries the Q staging group (S_QH's parity must stay the body's) — at the head of the ONE stream that owns M0:
                # the K / V groups of the fast bodies are not atomic, another stream writing M0 between their M0 write and their loads would misdirect them
                grp = self.qstage_group(par) + grp
            self.place(load, slots, grp, cfg["dma"][0], cfg["dma"][1], 2)
        if s2 and "kread" not in abl and self.pool:
            self.place_pool_kreads(load, slots, par)
        elif s2 and "kread" not in abl:
            self.place(load, slots, self.stream_kread(par), cfg["kread"][0], cfg["kread"][1], 3)
        if s1 and "vread" not in abl:
            self.place(load, slots, self.stream_vread(par ^ 1), cfg["vread"][0], cfg["vread"][1], 4)
        if s1 and sumchk:
            self.place(load, slots, self.stream_exp_sum(1, par ^ 1), cfg["se1"][0], cfg["se1"][1], 1)
            self.place(load, slots, self.stream_pack(0, par ^ 1), cfg["sc0"][0], cfg["sc0"][1], 5)
            self.place(load, slots, self.stream_pack(1, par ^ 1), cfg["sc1"][0], cfg["sc1"][1], 6)
        elif s1 and "exp" not in abl:
            self.place(load, slots, self.stream_exp(0, par ^ 1), ew[0], ew[1] - 1.0, 5)
            self.place(load, slots, self.stream_exp(1, par ^ 1), ew[0], ew[1], 6)
        if qpre:
            assert not s1 and not s2          # (the scratch registers of the softmax streams)
            self.place(load, slots, self.stream_qprescale(), 0, ng, 8)
        for g in range(ng):
            slots[g].sort(key=lambda x: (x[0], x[1]))
        # sum-check bodies: where did each q block's check land?  Its rare block rewrites the C tuple CT[qb] that the MFMAs 32 + 2 qb (+1) read
        # (first QK^T k-step of the next tile); a check in a later gap leaves those scores at the old reference -> `fix` (S_FIX, rare_fix)
        for (lab, qb, rpar) in self.pending_rare_sum:
            gap = [g for g in range(ng) for (_, _, it) in slots[g] if isinstance(it, list) and any(
                x.op == "s_cbranch_vccnz" and x.ops[0].name == lab for x in it)]
            assert len(gap) == 1, (lab, gap)
            # PV(t) of this q block (MFMAs 16 qb .. 16 qb + 15) must be issued: the rare block rescales its accumulators
            assert gap[0] >= (self.npv // 2) * (qb + 1) - 1, "sum check of q block %d in gap %d: its PV MFMAs are not all issued" % (qb, gap[0])
            ct_first, ct_last = self.ct_reader_gaps(qb)
            if self.ct:
                # `fix` treats the first-k-step MFMAs of this q block (gaps ct_first .. ct_last) as one event: a check between them would rewrite the C
                # tuple for some of the scores only, and rare_fix shifts all of them — refuse such a schedule
                assert not (ct_first <= gap[0] < ct_last), "sum check of q block %d in gap %d: between the MFMAs that read its C tuple" % (qb, gap[0])
            # the pair packing of this q block (stream_pack) rounds P in place; the rare block reads the unpacked f32 P -> no pack instruction ahead of the check
            packs = [(g, pos) for g in range(ng) for (pos, sid, it) in slots[g] if sid == 5 + qb and not isinstance(it, list) and it.op == self.cvt]
            chk = [(g, pos) for g in range(ng) for (pos, sid, it) in slots[g] if isinstance(it, list) and any(
                x.op == "s_cbranch_vccnz" and x.ops[0].name == lab for x in it)]
            assert packs and min(packs) > chk[0], "pair packing of q block %d starts at %s, ahead of its sum check at %s" % (qb, min(packs), chk[0])
            self.rare.append(self.rare_sum(lab, qb, rpar, fix=self.ct and gap[0] >= ct_last))
            self.check_gaps[(name, qb)] = gap[0]
        # emit: gap g fillers come AFTER mfma g
        body_start = len(p.ins)
        for g in range(ng):
            if g == self.npv and sumchk:
                # (no pending O rescale can exist in a sum-check fast body: its rare blocks rescale at once, the head body before it sets no flag)
                if s2 and "wait32" not in abl:
                    p.emit("s_waitcnt", lgkmcnt=0)
                if trace:
                    p.emit("s_memtime", S_TB)
            elif g == self.npv:
                # phase boundary: all of PV(t) is issued.  Rare O rescale, then K(t+2) fragments must have landed.
                lab = p.fresh("rare_r")
                p.emit("s_cmp_lg_u32", S_FLAG, 0)
                p.emit("s_cbranch_scc1", Label(lab))
                p.label(lab + "_ret")
                self.rare.append(self.rare_rescale(lab))
                if s2 and "wait32" not in abl:
                    p.emit("s_waitcnt", lgkmcnt=0)
                if trace:
                    p.emit("s_memtime", S_TB)
            if mf[g] is not None:
                p.ins.append(mf[g])
            for (_, _, item) in slots[g]:
                p.ins.extend(item if isinstance(item, list) else [item])
        if self.pool:
            p.ins[body_start:] = self.lds_waits(p.ins[body_start:])
        self.body_end(par, name, fast and not abl, s1)
        # end of body: DMA landed, my LDS reads done, then everybody
        p.emit("s_add_u32", S_T, S_T, 1)
        p.emit("s_add_u32", S_KOFF, S_KOFF, A_KTILE)
        p.emit("s_add_u32", S_VOFF, S_VOFF, A_VTILE)
        if "waitend" not in abl and guarded and dma:
            # (bodies that may have staged the next item's tiles: those loads are waited for by the next statement)
            lab = p.fresh("novm")
            p.emit("s_cmp_eq_u32", S_NOVM, 0)
            p.emit("s_cbranch_scc0", Label(lab))
            p.emit("s_waitcnt", vmcnt=0)
            p.label(lab)
            p.emit("s_waitcnt", lgkmcnt=0)
        elif "waitend" not in abl:
            p.emit("s_waitcnt", vmcnt=0, lgkmcnt=0)
        if trace:
            p.emit("s_memtime", S_TC)
        if "barrier" not in abl:
            p.emit("s_barrier")
        if tkind is not None:
            p.emit("s_memtime", S(84, 2))
            p.emit("s_waitcnt", lgkmcnt=0)
            p.emit("s_sub_u32", S_TMP, S(84), S_TA[0])
            p.emit("s_add_u32", S_SUM[tkind], S_SUM[tkind], S_TMP)
        if trace:       # sums of the low words: PV phase, QK phase (+ end-of-body wait), barrier
            p.emit("s_memtime", S(84, 2))
            p.emit("s_waitcnt", lgkmcnt=0)
            p.emit("s_sub_u32", S_TMP, S_TB[0], S_TA[0])
            p.emit("s_add_u32", S_SUM[0], S_SUM[0], S_TMP)
            p.emit("s_sub_u32", S_TMP, S_TC[0], S_TB[0])
            p.emit("s_add_u32", S_SUM[1], S_SUM[1], S_TMP)
            p.emit("s_sub_u32", S_TMP, S(84), S_TC[0])
            p.emit("s_add_u32", S_SUM[2], S_SUM[2], S_TMP)
            p.emit("s_add_u32", S_SUM[3], S_SUM[3], 1)

    _regs = staticmethod(sched.regs)

    def lds_waits(self, items, look=3):
        return sched.lds_waits(items, look)

    def rare_rescale(self, lab):
        r = [Ins("label", (Label(lab),))]
        r.append(mk("s_nop", 15))
        r.append(mk("s_nop", 15))
        for qb in range(2):
            skip = self.p.fresh("rr_skip")
            r.append(mk("s_bitcmp1_b32", S_FLAG, qb))
            r.append(mk("s_cbranch_scc0", Label(skip)))
            for dt in range(self.g.NDT):
                acc = self.oacc(qb, dt)
                for i in range(0, 16, 8):
                    for j in range(8):
                        r.append(mk("v_accvgpr_read_b32", TMP[j], acc[i + j]))
                    r.append(mk("s_nop", 1))
                    for j in range(8):
                        r.append(mk("v_mul_f32", TMP[j], TMP[j], FSC[qb]))
                    r.append(mk("s_nop", 1))
                    for j in range(8):
                        r.append(mk("v_accvgpr_write_b32", acc[i + j], TMP[j]))
            r.append(Ins("label", (Label(skip),)))
        r.append(mk("s_mov_b32", S_FLAG, 0))
        r.append(mk("s_nop", 7))
        r.append(mk("s_branch", Label(lab + "_ret")))
        return r

    # ------------------------------------------------------------------ whole block
    def epilogue_row_sum(self, qb):
        """Both epilogues: the row sum l of q block qb (two chains, two lane halves), its log2-domain LSE parked in KD[qb] (the outputs may share
        registers with inputs: they are written last).  Returns the register that holds 1 / l."""
        p = self.p
        lt, t, inv = EP_LT, EP_T, EP_INV
        p.emit("v_add_f32", lt, LA[qb], LB[qb])
        p.emit("s_nop", 0)
        p.emit("v_mov_b32", t, lt)
        p.emit("s_nop", 1)
        p.emit("v_permlane32_swap_b32", lt, t)
        p.emit("v_add_f32", lt, lt, t)
        p.emit("s_nop", 0)
        p.emit("v_rcp_f32", inv, lt)
        p.emit("v_log_f32", t, lt)
        p.emit("s_nop", 0)
        p.emit("v_add_f32", KD[qb], MC[qb], t)
        return inv

    def build(self):
        p = self.p
        tr = int(self.cfg["trace"][0])
        # ---- entry: constants, state, Q fragments, K(0)
        p.emit("s_waitcnt", vmcnt=0, lgkmcnt=0)
        if tr:
            p.emit("s_memtime", S_MARK[0])
        g = self.g
        for ks in range(g.NKS):
            p.emit("v_xor_b32", KR[ks], ks << 5, A_KR0)
        for dt in range(g.NDT):
            p.emit("v_xor_b32", VR[dt], dt << 6, A_VR0)
        # The wave's 64 Q rows: LDS-DMA into its part of the epilogue image (four 16-row groups of NP pieces, whole rows per instruction), unless the
        # previous item of this persistent workgroup staged them and read them into the fragment registers at its seam (flag bit 0)
        p.emit("s_lshr_b32", S_WAVE, A_LDSW, (g.SLOT_B // 4).bit_length() - 1)
        p.emit("s_mul_i32", S_QSB, S_WAVE, 64 * g.EPI_ROWB)
        p.emit("s_add_u32", S_QSB, S_QSB, g.EPI_BASE)
        # source offsets of piece i of a group: rows RPP * i further down, the granule swizzle follows the row (xor i << 6), the instruction offset that
        # selects the LDS piece is taken back out of the source address (like KD / VD below)
        p.emit("v_mov_b32", QD[0], A_QD0)
        p.emit("s_lshr_b32", S_TMP2, A_QT16, (16 // g.RPP).bit_length() - 1)       # RPP * Q row bytes
        p.emit("s_sub_u32", S_TMP2, S_TMP2, 1024)
        p.emit("s_mov_b32", S_TMP, 0)
        for i in range(1, g.NP):
            p.emit("s_add_u32", S_TMP, S_TMP, S_TMP2)
            p.emit("v_xor_b32", QD[i], i << 6, A_QD0)
            p.emit("s_nop", 0)
            p.emit("v_add_u32", QD[i], S_TMP, QD[i])
        p.emit("s_and_b32", S_PF, A_FLAGS, 1)
        p.emit("s_cmp_eq_u32", S_PF, 1)
        p.emit("s_cbranch_scc1", Label("have_q"))
        p.emit("s_mov_b32", S_TMP, A_QW)
        for j in range(4):
            p.emit("s_add_u32", M0, S_QSB, j * g.NP * 1024)
            if j:
                p.emit("s_add_u32", S_TMP, S_TMP, A_QT16)
            else:
                p.emit("s_nop", 0)
            for ins in self.q_group_loads(A_QRS, S_TMP):
                p.ins.append(ins)
        nq = 4 * g.NKS              # registers of one q block's fragments
        qv = V(VBASE, 2 * nq)
        if not self.fold:
            p.label("have_q")
        else:
            # folded scale: Q comes through the (still unused) S banks, is multiplied by c in f32 and rounded back ONCE —
            # the reference oracle's contract `scale * q_frags` (pure_torch_ver.py:61) — then parked in the accumulator file
            if self.qpre:      # (a prefetched item's fragments were prescaled in place by the previous item's last body: stream_qprescale)
                p.label("have_q")
            else:
                p.emit("s_branch", Label("q_issued"))
                p.label("have_q")
                for i in range(2 * nq):       # prefetched raw Q sits in the fragment registers: back through the S banks for the prescale
                    qreg = self.qf(i // nq, (i % nq) // 4)[i % 4]
                    p.emit("v_accvgpr_read_b32", V(VBASE + i), qreg)
                p.label("q_issued")
        # DMA source offsets of piece i: rows 4*i further down, the K granule swizzle follows the row (xor i<<6), and the
        # instruction offset 1024*i that selects the LDS piece is taken back out of the source address
        p.emit("v_mov_b32", KD[0], A_KD0)
        p.emit("v_mov_b32", VD[0], A_VD0)
        p.emit("s_mov_b32", S_TMP, 0)
        p.emit("s_mov_b32", S_TMP2, 0)
        for i in range(1, g.NP):
            p.emit("s_add_u32", S_TMP, S_TMP, A_KROW4)
            p.emit("s_add_u32", S_TMP2, S_TMP2, A_VROW4)
            p.emit("v_xor_b32", KD[i], i << 6, A_KD0)
            p.emit("v_add_u32", VD[i], S_TMP2, A_VD0)
            p.emit("s_nop", 0)
            p.emit("v_add_u32", KD[i], S_TMP, KD[i])
        p.emit("s_mov_b32", S_T, -2)
        p.emit("s_mov_b32", S_FLAG, 0)
        p.emit("s_mov_b32", S_FIX, 0)
        for r in S_SUM:
            p.emit("s_mov_b32", r, 0)
        p.emit("s_mov_b32", S_KOFF, 0)
        p.emit("s_mov_b32", S_NOVM, 0)
        p.emit("s_mov_b32", S_VOFF, 0)
        p.emit("s_cmp_eq_u32", S_PF, 1)
        p.emit("s_cbranch_scc1", Label("staged"))
        # K(0) -> K slot 0 (always exists)
        p.emit("s_add_u32", M0, A_LDSW, g.K_SLOT)
        p.emit("s_nop", 0)
        for i in range(g.NP):
            p.emit("buffer_load_dwordx4", KD[i], A_KRS, S_KOFF, offen=True, offset=1024 * i, lds=True)
        # ... and what body B(-2) would stage, V(0) and K(1), right behind it: all three tiles' latencies overlap (B(-2) then
        # stages nothing).  The running offsets are those of tile t+3 / t+2 of the body that uses them.
        p.emit("s_add_u32", M0, A_LDSW, g.V_BASE)
        p.emit("s_nop", 0)
        for i in range(g.NP):
            p.emit("buffer_load_dwordx4", VD[i], A_VRS, S_VOFF, offen=True, offset=1024 * i, lds=True)
        p.emit("s_cmp_lt_i32", A_NTWG, 2)
        p.emit("s_cbranch_scc1", Label("no_k1"))
        p.emit("s_add_u32", M0, A_LDSW, g.K_SLOT + g.SLOT_B)
        p.emit("s_nop", 0)
        for i in range(g.NP):
            p.emit("buffer_load_dwordx4", KD[i], A_KRS, A_KTILE, offen=True, offset=1024 * i, lds=True)
        p.label("no_k1")
        # Q (issued first: K(0), V(0) and K(1) — 3 or 2 x NP pieces behind it — keep flying) from the image into the fragment registers (f32-scale bodies) or
        # into the still unused S banks (folded scale: the prescale below)
        p.emit("s_cmp_lt_i32", A_NTWG, 2)
        p.emit("s_cbranch_scc1", Label("qwait8"))
        p.emit("s_waitcnt", vmcnt=3 * g.NP)
        p.emit("s_branch", Label("qwaited"))
        p.label("qwait8")
        p.emit("s_waitcnt", vmcnt=2 * g.NP)
        p.label("qwaited")
        for ks in range(g.NKS):
            p.emit("v_add_u32", TMP[ks], S_QSB, KR[ks])
        p.emit("s_nop", 0)
        for qb in range(2):
            for ks in range(g.NKS):
                p.emit("ds_read_b128", qv.sub(nq * qb + 4 * ks, 4) if self.fold else self.qf(qb, ks), TMP[ks], offset=qb * 32 * g.ROWB)
        p.label("staged")
        if tr == 8:
            p.emit("s_memtime", S_MARKH[1])
        # staging state of the NEXT item's Q (qstage_group): nothing staged yet, or nothing to stage
        p.emit("s_bitcmp1_b32", A_FLAGS, 1)
        p.emit("s_cselect_b32", S_QH, 0, 8)
        p.emit("s_mov_b32", S_QM0, S_QSB)
        p.emit("s_mov_b32", S_QSOFF, A_NQW)
        p.emit("s_mov_b32", S_KOFF, A_KTILE)     # the running offsets are those of tile t+3 / t+2 of the body that uses them
        for qb in range(2):
            p.emit("v_mov_b32", MC[qb], 0.0 if self.fold else NEG_INF)
            p.emit("v_mov_b32", LA[qb], 0)
            p.emit("v_mov_b32", LB[qb], 0)
            p.emit("v_mov_b32", FSC[qb], 1.0)
        for i in range(32 * g.NDT):
            p.emit("v_accvgpr_write_b32", A(i), 0)
        if self.ct:
            for qb in range(2):
                for i in range(16):
                    p.emit("v_mov_b32", CT[qb][i], 0)              # C tuples: the reference starts at 0
        if self.fold:
            if self.qpre:
                p.emit("s_cmp_eq_u32", S_PF, 1)
                p.emit("s_cbranch_scc1", Label("q_prescaled"))
            p.emit("s_waitcnt", lgkmcnt=0)                          # the Q reads from the image
            for i in range(8 * g.NKS):
                qreg = self.qf(i // (4 * g.NKS), (i % (4 * g.NKS)) // 4)[i % 4]
                for ins in self.q_prescale_reg(V(VBASE + i), qreg, TMP[2 * (i & 1)], TMP[2 * (i & 1) + 1]):
                    p.ins.append(ins)
            p.label("q_prescaled")
        # K(0) is needed now (and the Q reads); V(0) and K(1) (8 or 4 pieces issued behind it) may keep flying until the end of B(-2)
        p.emit("s_waitcnt", lgkmcnt=0)
        p.emit("s_cmp_lt_i32", A_NTWG, 2)
        p.emit("s_cbranch_scc1", Label("wait4"))
        p.emit("s_waitcnt", vmcnt=2 * g.NP)
        p.emit("s_branch", Label("waited"))
        p.label("wait4")
        p.emit("s_waitcnt", vmcnt=g.NP)
        p.label("waited")
        if tr:
            p.emit("s_memtime", S_MARKE)
        p.emit("s_barrier")
        if tr:
            p.emit("s_memtime", S_MARKH[0])

        # ---- head bodies: t = -2 (parity 0): QK(0) only; t = -1 (parity 1): softmax of tile 0, QK(1) if there is a tile 1
        self.body(0, pv=False, s1=False, s2=True, name="H1", dma=False)
        if tr and tr != 8:
            p.emit("s_memtime", S_MARKH[1])
        p.emit("s_cmp_eq_u32", A_NTW, 1)
        p.emit("s_cbranch_scc1", Label("h2b"))
        self.body(1, pv=False, s1=True, s2=True, name="H2", first=True)
        p.emit("s_branch", Label("main"))
        p.label("h2b")
        self.body(1, pv=False, s1=True, s2=False, masked=True, name="H2b", first=True)

        # ---- main: fast bodies while ntw - t >= 4 (then tile t+1 is not the last one and the staged tiles t+2, t+3 exist)
        p.label("main")
        if tr:
            p.emit("s_memtime", S_MARK[1])
        if self.sumchk:
            p.emit("s_bitcmp1_b32", A_FLAGS, 4)           # safe mode (the redo of an item whose sum check met a non-finite P): max-first bodies only
            p.emit("s_cbranch_scc1", Label("dispatch"))
        p.emit("s_sub_u32", S_NFAST, A_NTW, 3)            # number of fast bodies (t = 0 .. ntw-4), if positive
        p.emit("s_cmp_gt_i32", S_NFAST, 0)
        p.emit("s_cbranch_scc0", Label("dispatch"))
        p.emit("s_nop", 0)
        p.label("fast0")
        self.body(0, guarded=False, name="F0")
        p.emit("s_sub_u32", S_NFAST, S_NFAST, 1)
        p.emit("s_cmp_gt_i32", S_NFAST, 0)
        p.emit("s_cbranch_scc0", Label("dispatch"))
        self.body(1, guarded=False, name="F1")
        p.emit("s_sub_u32", S_NFAST, S_NFAST, 1)
        p.emit("s_cmp_gt_i32", S_NFAST, 0)
        p.emit("s_cbranch_scc1", Label("fast0"))

        p.label("dispatch")
        p.emit("s_cmp_ge_i32", S_T, A_NTWG)
        p.emit("s_cbranch_scc1", Label("epilogue"))
        p.emit("s_sub_u32", S_D, A_NTW, S_T)              # tiles left for this wave, the one PV'd next included
        p.emit("s_and_b32", S_TMP, S_T, 1)
        p.emit("s_cmp_eq_u32", S_TMP, 1)
        p.emit("s_cbranch_scc1", Label("disp_odd"))
        for par, suffix in ((0, "e"), (1, "o")):
            if par == 1:
                p.label("disp_odd")
            p.emit("s_cmp_ge_i32", S_D, 3)
            p.emit("s_cbranch_scc1", Label("ta_" + suffix))
            p.emit("s_cmp_eq_u32", S_D, 2)
            p.emit("s_cbranch_scc1", Label("tb_" + suffix))
            p.emit("s_cmp_eq_u32", S_D, 1)
            p.emit("s_cbranch_scc1", Label("tc_" + suffix))
            if self.qpre:
                self.qpre_check("stq_" + suffix)
            self.body(par, pv=False, s1=False, s2=False, name="ST%d" % par)     # this wave is done: stage + sync only
            p.emit("s_branch", Label("dispatch"))
            if self.qpre:
                p.label("stq_" + suffix)
                self.body(par, pv=False, s1=False, s2=False, name="STQ%d" % par, qpre=True)
                p.emit("s_branch", Label("dispatch"))
            p.label("ta_" + suffix)
            self.body(par, name="TA%d" % par)                                   # like a fast body, staging guarded
            p.emit("s_branch", Label("dispatch"))
            p.label("tb_" + suffix)
            self.body(par, s2=False, masked=True, name="TB%d" % par)            # tile t+1 is the last: masks
            p.emit("s_branch", Label("dispatch"))
            p.label("tc_" + suffix)
            if self.qpre:
                self.qpre_check("tcq_" + suffix)
            self.body(par, s1=False, s2=False, name="TC%d" % par)
            if self.qpre:
                p.emit("s_branch", Label("dispatch"))
                p.label("tcq_" + suffix)
                self.body(par, s1=False, s2=False, name="TCQ%d" % par, qpre=True)
            p.emit("s_branch", Label("dispatch"))

        # ---- epilogue: O / l -> 16 bit -> wave-private LDS image (rows of 272 B); LSE out
        p.label("epilogue")
        if tr:
            p.emit("s_memtime", S_MARK[2])
        p.emit("s_nop", 15)
        p.emit("s_bitcmp1_b32", A_FLAGS, 3)
        p.emit("s_cbranch_scc1", Label("epilogue_part"))
        for qb in range(2):
            inv = self.epilogue_row_sum(qb)
            for dt in range(g.NDT):
                acc = self.oacc(qb, dt)
                for r4 in (0, 2):
                    for j in range(8):
                        p.emit("v_accvgpr_read_b32", TMP[j], acc[4 * r4 + j])
                    p.emit("s_nop", 0)
                    for j in range(8):
                        p.emit("v_mul_f32", TMP[j], TMP[j], inv)
                    p.emit("s_nop", 0)
                    # a0, a1 = regs 4r4+0..3, b0, b1 = regs 4r4+4..7, packed into four consecutive scratch registers
                    d4 = V(TMP[0].idx, 4)
                    assert [TMP[j].idx for j in range(4)] == [d4.idx + j for j in range(4)]
                    p.emit(self.cvt, TMP[0], TMP[0], TMP[1])
                    p.emit(self.cvt, TMP[1], TMP[2], TMP[3])
                    p.emit(self.cvt, TMP[2], TMP[4], TMP[5])
                    p.emit(self.cvt, TMP[3], TMP[6], TMP[7])
                    p.emit("s_nop", 1)
                    p.emit("v_permlane32_swap_b32", TMP[0], TMP[2])
                    p.emit("v_permlane32_swap_b32", TMP[1], TMP[3])
                    p.emit("s_nop", 0)
                    # 16 bytes {x0[0], x1[0], x0[1], x1[1]} at row (32qb + l31), column 32dt + 8(r4 + hi)
                    p.emit("ds_write_b128", A_EPI, d4, offset=32 * qb * g.EPI_ROWB + (32 * dt + 8 * r4) * 2)
                    p.emit("s_nop", 1)
        p.emit("s_waitcnt", lgkmcnt=0)
        p.emit("v_mov_b32", A_LSE0, KD[0])
        p.emit("v_mov_b32", A_LSE1, KD[1])
        if tr:          # developer build: the LSE outputs carry cycle counts instead
            p.emit("s_memtime", S_MARK[3])
            p.emit("s_waitcnt", lgkmcnt=0)
            if tr == 1:      # PV-phase and QK-phase sums over the fast bodies
                a, b = S_SUM[0], S_SUM[1]
            elif tr == 2:    # barrier sum, number of fast bodies
                a, b = S_SUM[2], S_SUM[3]
            elif tr == 3:    # entry -> first main body, epilogue
                p.emit("s_sub_u32", S_TMP, S_MARK[1][0], S_MARK[0][0])
                p.emit("s_sub_u32", S_TMP2, S_MARK[3][0], S_MARK[2][0])
                a, b = S_TMP, S_TMP2
            elif tr == 5:    # entry -> past the entry barrier, that barrier -> end of the first head body
                p.emit("s_sub_u32", S_TMP, S_MARKH[0][0], S_MARK[0][0])
                p.emit("s_sub_u32", S_TMP2, S_MARKH[1][0], S_MARKH[0][0])
                a, b = S_TMP, S_TMP2
            elif tr == 9:    # tail bodies: TA, TB
                a, b = S_SUM[0], S_SUM[1]
            elif tr == 10:   # tail bodies: TC, ST
                a, b = S_SUM[2], S_SUM[3]
            elif tr == 8:    # entry -> the "staged" label (address set-up, Q / first tiles issued unless prefetched), from there to the entry barrier (state, zeroed accumulators, prescale, wait)
                p.emit("s_sub_u32", S_TMP, S_MARKH[1][0], S_MARK[0][0])
                p.emit("s_sub_u32", S_TMP2, S_MARKE[0], S_MARKH[1][0])
                a, b = S_TMP, S_TMP2
            elif tr == 7:    # entry -> in front of the entry barrier, waiting at that barrier
                p.emit("s_sub_u32", S_TMP, S_MARKE[0], S_MARK[0][0])
                p.emit("s_sub_u32", S_TMP2, S_MARKH[0][0], S_MARKE[0])
                a, b = S_TMP, S_TMP2
            elif tr == 6:    # second head body, tail bodies (main bodies minus ... see trace 4 / 1)
                p.emit("s_sub_u32", S_TMP, S_MARK[1][0], S_MARKH[1][0])
                p.emit("s_sub_u32", S_TMP2, S_MARK[2][0], S_MARK[1][0])
                a, b = S_TMP, S_TMP2
            else:            # whole block, main bodies (fast + tail)
                p.emit("s_sub_u32", S_TMP, S_MARK[3][0], S_MARK[0][0])
                p.emit("s_sub_u32", S_TMP2, S_MARK[2][0], S_MARK[1][0])
                a, b = S_TMP, S_TMP2
            p.emit("v_cvt_f32_u32", A_LSE0, a)
            p.emit("v_cvt_f32_u32", A_LSE1, b)
        # out-of-line blocks
        p.emit("s_branch", Label("end"))
        # ---- epilogue of a KV-split part: O / l in f32 straight to the workspace tile (see A_WSB), LSE out
        p.label("epilogue_part")
        # this lane's place in the tile: (64 * wave + l31) * 32 + hi * 16 bytes (the lane id from v_mbcnt: no operand register left for it)
        p.emit("v_mbcnt_lo_u32_b32", TMP[0], -1, 0)
        p.emit("v_mbcnt_hi_u32_b32", TMP[0], -1, TMP[0])
        p.emit("s_lshl_b32", S_TMP, S_WAVE, 6)
        p.emit("v_and_b32", TMP[1], 31, TMP[0])
        p.emit("v_lshrrev_b32", TMP[2], 5, TMP[0])
        p.emit("v_add_u32", TMP[1], S_TMP, TMP[1])
        p.emit("v_lshlrev_b32", TMP[2], 4, TMP[2])
        p.emit("v_lshlrev_b32", TMP[1], 5, TMP[1])
        p.emit("s_nop", 0)
        p.emit("v_add_u32", WSO, TMP[1], TMP[2])
        for qb in range(2):
            inv = self.epilogue_row_sum(qb)
            for dt in range(g.NDT):
                acc = self.oacc(qb, dt)
                for r4 in (0, 2):
                    for j in range(8):
                        p.emit("v_accvgpr_read_b32", TMP[j], acc[4 * r4 + j])
                    p.emit("s_nop", 0)
                    for j in range(8):
                        p.emit("v_mul_f32", TMP[j], TMP[j], inv)
                    for half in range(2):          # registers 4*r4 + 4*half .. +3  <->  g = r4 + half
                        p.emit("v_add_u32", KD[2 + half], 1024 * qb + 8192 * (4 * dt + r4 + half), WSO)
                    p.emit("s_nop", 0)
                    for half in range(2):
                        p.emit("global_store_dwordx4", KD[2 + half], V(TMP[4 * half].idx, 4), A_WSB)
                    p.emit("s_nop", 3)             # (a store of more than 64 bits: its data registers must not be rewritten right behind it)
        p.emit("s_waitcnt", vmcnt=0, lgkmcnt=0)     # the stores, and whatever the item seam prefetched: the next statement counts loads only
        p.emit("v_mov_b32", A_LSE0, KD[0])
        p.emit("v_mov_b32", A_LSE1, KD[1])
        p.emit("s_branch", Label("end"))
        for r in self.rare:
            p.extend(r)
        p.label("end")
        return p




def main():
    # Two bodies per (head dim, dtype), chosen per launch by the host (host.cpp: plan_range; option "fold"):
    #   fa2_fwd_d<hd>_<dt>.inc       the scale multiplies the f32 Q.K^T product — the reference kernel's contract (kernel_fp16.cu:164)
    #   fa2_fwd_d<hd>_<dt>_fold.inc  "ct": Q * scale*log2e rounded once to the I/O dtype — the scaling contract of the reference's own oracle,
    #                                pure_torch_ver.py:61 — and the running reference enters the first QK^T k-step as its C operand: the 64
    #                                v_fma_f32 per tile go.  Head dim 64, whose body runs at its issue bound: +9 % (B2 H16 N4096); head dim 128:
    #                                +1.4 % config 2, +2.1 % config 4, +2.9 % B8 (tools/kbench.py, one box).  fp16: ~2e-4 of log2 LSE on U[0,1) /
    #                                N(0,1) inputs, growing with the logits; bf16 (8-bit mantissa): ~6e-3 — opt-in only (option "fold" = 2).
    variants = [("fa2_fwd_d%d_%s%s.inc" % (hd, "bf16" if bf16 else "f16", "_fold" if fold else ""), Gen, {"bf16": bf16, "hd": hd}, ("ct",) if fold else ())
                for hd in (128, 64) for bf16 in (False, True) for fold in (False, True)]
    gen_driver.run("fwd_d128_gen.py", variants, managed=("f32scale", "ct"), clobbers=[("fa2_fwd_d128_clobbers.inc", VBASE, CLOBBER_S)])


if __name__ == "__main__":
    main()
