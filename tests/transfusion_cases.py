"""Float64 yardsticks and generated inputs for the TransFusion head's own device kernels (csrc/proposals.hip,
tok_mha16_kernel / tok_mha16_combine_kernel of csrc/tok_attention.h and csrc/tok_shared.h), shared by the GPU test
(tests/test_transfusion_edges_gpu.py) and the CPU checks of the yardsticks and premises (tests/test_transfusion_cases_cpu.py).
numpy only, plus torch for the float32 evaluation of the attention expression; every case comes from a fixed seed.

``proposals_ref`` states the kernel's documented rule: score = float32(sigmoid in float64); a cell is a peak iff no
neighbour of its k x k window is LARGER (interior cells only: the k//2 frame never proposes); free classes propose at every
cell; winners = the P largest masked scores ordered by (score descending, flat index ``c * HW + cell`` ascending).

THE LOGIT ALPHABETS.  The kernel's sigmoid is ``1 / (1 + expf(-x))`` in float32; it need not round like the yardstick's.
The cases therefore draw logits from sets on which any sigmoid good to a few hundred ulp gives the same ORDER and the
same ties, so that class and cell compare with ``array_equal``:

  quarter steps   j / 4, |j| <= 32: 65 values whose float32 sigmoids are >= 1,597 ulp apart -- and ties everywhere
  saturation      {-inf, <= -200, 0, >= 40, +inf}: scores exactly 0, 0.5 and 1 in both precisions (nothing in (-104, -87),
                  where the float32 score is denormal)
  fine ladder     j * 2^-19, j < 256, one value per cell of one class, all else -inf: scores 8 ulp apart that share key
                  bits 31 .. 11, so only radix passes 2 and 3 of the select can order them (the GPU test asserts on the
                  kernel's own scores that they increase strictly with j before it asserts the order)
"""
import functools

import numpy as np

TP_THREADS = 1024       # csrc/proposals.hip: threads of the select workgroup = index chunks of the collect step
TP_MAXP = 256           # csrc/proposals.hip: the most proposals
MHA_CHUNK = 1024        # tok_mha16_plan: the most keys per chunk
LADDER_STEP = 2.0 ** -19


# ------------------------------------------------------------------------------------------------------- proposals
def sigmoid32(logits):
    """float32(sigmoid evaluated in float64)."""
    with np.errstate(over="ignore"):
        return (1.0 / (1.0 + np.exp(-np.asarray(logits, np.float64)))).astype(np.float32)


def masked_scores(logits, k, free):
    """logits [H, W, C] -> masked scores [C, H * W] float32 (0 where the cell does not propose the class)."""
    H, W, C = logits.shape
    score = sigmoid32(logits).transpose(2, 0, 1)                      # [C, H, W]
    r = k // 2
    larger = np.zeros(score.shape, bool)                              # some neighbour of the window is larger
    inner = score[:, r:H - r, r:W - r]
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            if dy or dx:
                larger[:, r:H - r, r:W - r] |= score[:, r + dy:H - r + dy, r + dx:W - r + dx] > inner
    peak = np.zeros(score.shape, bool)
    peak[:, r:H - r, r:W - r] = ~larger[:, r:H - r, r:W - r]
    for c in free:
        if c < C:
            peak[c] = True
    return np.where(peak, score, np.float32(0)).reshape(C, H * W)


def proposals_ref(logits, k, free, P):
    """One sample's logits [H, W, C] -> (class [P], cell [P], masked scores of the winning cells [C, P], number of positive
    masked scores).  Ties resolve towards the smaller flat index (a stable sort of the negated scores)."""
    H, W, C = logits.shape
    masked = masked_scores(logits, k, free)
    flat = masked.reshape(-1)
    order = np.argsort(-flat.astype(np.float64), kind="stable")[:P]
    cls, cell = order // (H * W), order % (H * W)
    return cls.astype(np.int64), cell.astype(np.int64), masked[:, cell], int((flat > 0).sum())


def quarter_steps(rng, shape):
    return (rng.integers(-32, 33, size=shape) * 0.25).astype(np.float32)


NUSC = (8, 9)
ALL10 = tuple(range(10))
PROPOSAL_CASES = (
    "P1", "P2", "P200", "P255", "P256", "N_eq_P", "N1023", "N1024", "N1025", "N2049", "C1", "C32", "k5_9x11", "k3_3x3", "k5_5x7",
    "const_free", "const_plateau", "ties_waves", "peaks_out", "saturation", "ladder", "B3", "workload")


@functools.lru_cache(maxsize=None)
def proposal_case(name):
    """-> dict(logits [B, H, W, C] f32, k, free, P) (+ what a family adds).  Quarter-step logits unless the name says else."""
    rng = np.random.default_rng(sum(map(ord, name)))
    B, k, free, P = 1, 3, NUSC, 200
    extra = {}
    if name in ("P1", "P2", "P200", "P255", "P256"):
        H, W, C, P = 9, 11, 10, int(name[1:])
    elif name == "N_eq_P":
        H, W, C, free = 5, 5, 8, ()                                   # N = 200 = P: every key wins, the zeros included
    elif name == "N1023":
        H, W, C = 3, 11, 31
    elif name == "N1024":
        H, W, C = 4, 8, 32
    elif name == "N1025":
        H, W, C, free = 5, 41, 5, ()
    elif name == "N2049":
        H, W, C, free = 3, 683, 1, ()                                 # 2 * 1024 + 1: a thread chunk of 3, the last one short
    elif name == "C1":
        H, W, C, free, P = 9, 11, 1, (), 64
    elif name == "C32":
        H, W, C, free = 9, 11, 32, (31,)                              # bit 31 of the free-class mask
    elif name == "k5_9x11":
        H, W, C, k = 9, 11, 10, 5
    elif name == "k3_3x3":
        H, W, C, P = 3, 3, 10, 40                                     # one interior cell
    elif name == "k5_5x7":
        H, W, C, k = 5, 7, 10, 5
    elif name in ("const_free", "const_plateau"):
        H, W, C = 9, 11, 10
        free = ALL10 if name == "const_free" else ()
    elif name == "ties_waves":
        H, W, C, free = 32, 32, 10, ALL10
    elif name == "peaks_out":
        H, W, C, free = 5, 5, 10, ()                                  # at most 3 * 3 * 10 = 90 positive scores
    elif name == "saturation":
        H, W, C = 9, 11, 10
    elif name == "ladder":
        H, W, C, free = 16, 16, 3, (1,)
    elif name == "B3":
        B, H, W, C = 3, 9, 11, 10
    elif name == "workload":
        H, W, C = 180, 180, 10
    else:
        raise KeyError(name)
    logits = quarter_steps(rng, (B, H, W, C))
    if name.startswith("const"):
        logits[:] = 1.0
    elif name == "ties_waves":
        # 100 cells above the threshold value, 300 cells AT it, every other cell below: need = 100 of the 300, which lie 34
        # flat indices apart -- a wave of the collect step owns 64 chunks of 10 indices, so the 100 taken ties span six waves
        N = C * H * W
        tie = np.arange(300) * 34 + 5
        above = np.setdiff1d(np.arange(N), tie)[rng.permutation(N - 300)[:100]]
        flat = np.full(N, -8.0, np.float32)
        flat[tie], flat[above] = 2.0, 4.0
        logits = flat.reshape(C, H, W).transpose(1, 2, 0)[None].copy()
        extra = dict(tie=tie, above=np.sort(above), need=100)
    elif name == "saturation":
        alphabet = np.array([-np.inf, -200.0, -1e4, 0.0, 40.0, 1e4, np.inf], np.float32)
        logits = alphabet[rng.integers(0, len(alphabet), size=(B, H, W, C))]
    elif name == "ladder":
        logits[:] = -np.inf
        perm = rng.permutation(H * W)                                 # cell of ladder value j
        lad = np.empty(H * W, np.float32)
        lad[perm] = (np.arange(H * W) * LADDER_STEP).astype(np.float32)
        logits[0, :, :, 1] = lad.reshape(H, W)
        extra = dict(cell_of_j=perm)
    return dict(logits=np.ascontiguousarray(logits), k=k, free=free, P=P, **extra)


def nan_case():
    """Quarter-step logits on 9 x 11 x 10 with NaN at five cells that may propose: four interior cells and one frame cell of
    a free class.  -> (case dict, flat indices of the NaN keys ascending)."""
    c = dict(proposal_case("P200"))
    logits = c["logits"].copy()
    H, W = logits.shape[1:3]
    spots = [(0, 4, 5), (3, 1, 1), (3, 1, 2), (7, 7, 9), (9, 0, 0)]   # (class, y, x); the last on the frame of free class 9
    for cl, y, x in spots:
        logits[0, y, x, cl] = np.nan
    c["logits"] = logits
    return c, np.array(sorted(cl * H * W + y * W + x for cl, y, x in spots))


# ------------------------------------------------------------------------------------------------------- attention
def mha16_plan(Pq, Pk):
    """Mirror of tok_mha16_plan (csrc/tok_attention.h): (qtiles, chunks, keys_per_chunk)."""
    qtiles = (Pq + 31) // 32
    nchunk = (Pk + MHA_CHUNK - 1) // MHA_CHUNK
    kpc = (-(-Pk // nchunk) + 31) // 32 * 32
    return qtiles, -(-Pk // kpc), kpc


def mha16_ref(q, k, v, B, Pq, Pk, heads, scale):
    """softmax(q scale k^T) v per (sample, head) over 16-channel heads; q [B * Pq, heads * 16], k / v [B * Pk, heads * 16].
    -> (float64 numpy [B * Pq, heads * 16], the same expression in torch float32 as numpy)."""
    import torch

    def split(x, L):
        return np.asarray(x, np.float64).reshape(B, L, heads, 16).transpose(0, 2, 1, 3)
    logit = np.einsum("bhqd,bhkd->bhqk", split(q, Pq) * float(scale), split(k, Pk))
    w = np.exp(logit - logit.max(-1, keepdims=True))
    w /= w.sum(-1, keepdims=True)
    ref = np.einsum("bhqk,bhkd->bhqd", w, split(v, Pk)).transpose(0, 2, 1, 3).reshape(B * Pq, heads * 16)

    def t32(x, L):
        return torch.from_numpy(np.ascontiguousarray(x, np.float32)).reshape(B, L, heads, 16).permute(0, 2, 1, 3)
    w32 = torch.softmax((t32(q, Pq) * float(scale)) @ t32(k, Pk).transpose(-1, -2), dim=-1)
    ref32 = (w32 @ t32(v, Pk)).permute(0, 2, 1, 3).reshape(B * Pq, heads * 16).numpy()
    return ref, ref32


MHA_REGIMES = ("k0", "dom_first", "dom_last", "dom_chunk2", "rising", "falling")


def dominant_key(regime, Pk):
    """Key index of the dominant key: 0, the last key (in the partial tile), the first key of the second chunk (of the
    second tile where one chunk holds every key)."""
    _, chunks, kpc = mha16_plan(1, Pk)
    return {"dom_first": 0, "dom_last": Pk - 1, "dom_chunk2": kpc if chunks > 1 else 32}[regime]


def mha_case(regime, B, Pq, Pk, heads, seed=0):
    """-> (q [B * Pq, heads * 16], k, v [B * Pk, heads * 16]) float32, scale = 0.25.  ``random``: O(1) logits.  The known-answer
    regimes (q = 1 + 0.05 n in every channel, so a key whose 16 channels all hold t has logit ~ 4 t):
      k0         k = 0: uniform weights, the output is the mean of v over exactly Pk keys
      dom_*      one key at 15 per channel (logit ~ 60) over keys ~ 0.1 n: the output is that key's v row
      rising     key i holds (i // 32 + (i % 32) / 64) / 4 + 0.05 n: the logit rises by ~ 1 per 32-key tile (by ~ 0.5 inside
                 one), every tile raises the running max
      falling    the mirror image i -> Pk - 1 - i: the first tile holds the maximum, every later tile only adds to the sum"""
    rng = np.random.default_rng(1000 * Pq + Pk + 7 * heads + seed)
    C = heads * 16
    q = rng.standard_normal((B * Pq, C)) * 1.3
    k = rng.standard_normal((B * Pk, C)) * 1.3
    v = rng.standard_normal((B * Pk, C)) * 1.3
    if regime != "random":
        q = 1.0 + 0.05 * rng.standard_normal((B * Pq, C))
        key = np.tile(np.arange(Pk), B)[:, None]
        if regime == "k0":
            k = np.zeros((B * Pk, C))
        elif regime.startswith("dom_"):
            k = 0.1 * rng.standard_normal((B * Pk, C))
            k[key[:, 0] == dominant_key(regime, Pk)] = 15.0
        elif regime in ("rising", "falling"):
            i = key if regime == "rising" else Pk - 1 - key
            k = (i // 32 + (i % 32) / 64.0) / 4.0 + 0.05 * rng.standard_normal((B * Pk, C))
        else:
            raise KeyError(regime)
    return q.astype(np.float32), k.astype(np.float32), v.astype(np.float32)
