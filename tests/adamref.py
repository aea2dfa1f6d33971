"""numpy model of include/sfmi_optim.h, operation by operation: the float64 sum of squares in the header's fixed order, the state
block with its running products, the float32 element update -- and the bound that holds such a float32 trajectory to Adam in
float64 (profiles/device_adam.md has the derivation)."""
import numpy as np

f32, f64 = np.float32, np.float64
U32 = 2.0 ** -24   # float32's unit roundoff
CHUNK = 2048       # SF_OPT_CHUNK
MAX_TENSORS = 64   # SF_OPT_MAX_TENSORS
STATE_BYTES = 128  # SF_ADAM_STATE_BYTES

# sizes at which sf_adam_step takes another path: one element, around a wave, around a block's lanes, around the 1024 elements
# of a pass, around a chunk, several chunks and a tail that is no multiple of four
SIZES = (1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 5)


# ------------------------------------------------------------------------------------------------------------------ the norm
def chunk_partials(grad):
    """One float64 partial sum per chunk of a float32 tensor: lane l adds the squares of elements 4 l .. 4 l + 3, then of
    1024 + 4 l .. 1024 + 4 l + 3, in that order from 0.0 (beyond the end: +0.0); sf_fixed_sum.h's tree within each wave of 64
    lanes (lane l takes l ^ 32, ^ 16, ... ^ 1), the four waves in index order."""
    g = np.asarray(grad, f32).reshape(-1).astype(f64)
    n = g.size
    nch = (n + CHUNK - 1) // CHUNK
    sq = np.zeros(nch * CHUNK, f64)
    with np.errstate(all="ignore"):
        sq[:n] = g * g  # (exact: 24 x 24 bits)
        c = sq.reshape(nch, CHUNK // 1024, 256, 4)
        acc = np.zeros((nch, 256), f64)
        for p in range(CHUNK // 1024):
            for j in range(4):
                acc = acc + c[:, p, :, j]
        t = acc.reshape(nch, 4, 64)
        for off in (32, 16, 8, 4, 2, 1):
            t = t[..., :off] + t[..., off:2 * off]
        t = t[..., 0]
        return ((t[:, 0] + t[:, 1]) + t[:, 2]) + t[:, 3]


def sum_squares(grads):
    """S of the header: the chunks of all tensors in table order, one running sum from 0.0."""
    acc = f64(0)
    with np.errstate(all="ignore"):
        for g in grads:
            for b in chunk_partials(g):
                acc = acc + b
    return acc


def norm_coef(S, max_grad_norm):
    with np.errstate(all="ignore"):
        norm = np.sqrt(f64(S))
        coef = f64(1)
        if max_grad_norm is not None and max_grad_norm > 0:
            coef = min(f64(1), f64(max_grad_norm) / (norm + f64(1e-6)))
    return norm, coef


def total_chunks(sizes):
    return sum((int(n) + CHUNK - 1) // CHUNK for n in sizes)


# ------------------------------------------------------------------------------------------------------------ the state block
def new_state(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, t=0):
    """The state block after sf_adam_state_init (t = 0), or as load_state_dict rebuilds it at step t: t multiplications."""
    s = dict(t=0, beta1_pow=f64(1), beta2_pow=f64(1), lr=f64(lr), beta1=f64(beta1), beta2=f64(beta2), eps=f64(eps), norm=f64(0),
             coef=f64(0), skipped=0, scalars=np.zeros(8, f32), apply=0)
    for _ in range(t):
        s["beta1_pow"] = s["beta1_pow"] * s["beta1"]
        s["beta2_pow"] = s["beta2_pow"] * s["beta2"]
    s["t"] = t
    return s


def state_bytes(s):
    """The 128 bytes of the block."""
    b = np.zeros(STATE_BYTES, np.uint8)
    b[0:8] = np.array([s["t"]], np.int64).view(np.uint8)
    b[8:72] = np.array([s[k] for k in ("beta1_pow", "beta2_pow", "lr", "beta1", "beta2", "eps", "norm", "coef")], f64).view(np.uint8)
    b[72:80] = np.array([s["skipped"]], np.uint64).view(np.uint8)
    b[80:112] = np.asarray(s["scalars"], f32).view(np.uint8)
    b[112:116] = np.array([s["apply"]], np.uint32).view(np.uint8)
    return b


def parse_state(raw):
    """bytes [128] -> the dict"""
    b = np.frombuffer(np.ascontiguousarray(raw, np.uint8).tobytes(), np.uint8)
    d = b[8:72].view(f64)
    s = dict(zip(("beta1_pow", "beta2_pow", "lr", "beta1", "beta2", "eps", "norm", "coef"), (f64(x) for x in d)))
    s.update(t=int(b[0:8].view(np.int64)[0]), skipped=int(b[72:80].view(np.uint64)[0]), scalars=b[80:112].view(f32).copy(),
             apply=int(b[112:116].view(np.uint32)[0]), tail=b[116:].copy())
    return s


def states_equal(a, b):
    """Field by field; a NaN norm equals a NaN norm (the payloads of x86 and the GPU may differ)."""
    for k in ("t", "skipped", "apply"):
        if a[k] != b[k]:
            return False, k
    for k in ("beta1_pow", "beta2_pow", "lr", "beta1", "beta2", "eps", "norm", "coef"):
        x, y = f64(a[k]), f64(b[k])
        if not ((np.isnan(x) and np.isnan(y)) or x.tobytes() == y.tobytes()):
            return False, k
    if np.asarray(a["scalars"], f32).tobytes() != np.asarray(b["scalars"], f32).tobytes():
        return False, "scalars"
    return True, None


# -------------------------------------------------------------------------------------------------------------------- the step
def adam_step(state, params, grads, exp_avgs, exp_avg_sqs, max_grad_norm=None):
    """sf_adam_step -> (state', params', exp_avgs', exp_avg_sqs', stepped).  The inputs are not written."""
    s = dict(state)
    S = sum_squares(grads)
    s["norm"], coef = norm_coef(S, max_grad_norm)
    if not np.isfinite(S):
        s["coef"], s["apply"], s["skipped"] = f64(0), 0, s["skipped"] + 1
        return s, [p.copy() for p in params], [m.copy() for m in exp_avgs], [v.copy() for v in exp_avg_sqs], False
    s["t"] = s["t"] + 1
    s["beta1_pow"] = s["beta1_pow"] * s["beta1"]
    s["beta2_pow"] = s["beta2_pow"] * s["beta2"]
    bc1, bc2 = f64(1) - s["beta1_pow"], f64(1) - s["beta2_pow"]
    s["coef"], s["apply"] = coef, 1
    sc = np.array([f32(coef), f32(s["beta1"]), f32(f64(1) - s["beta1"]), f32(s["beta2"]), f32(f64(1) - s["beta2"]), f32(np.sqrt(bc2)),
                   f32(s["eps"]), f32(s["lr"] / bc1)], f32)
    s["scalars"] = sc
    c, b1, omb1, b2, omb2, sb, eps, step = (f32(x) for x in sc)
    P, M, V = [], [], []
    with np.errstate(all="ignore"):
        for p, gr, m, v in zip(params, grads, exp_avgs, exp_avg_sqs):
            p, gr, m, v = (np.asarray(x, f32) for x in (p, gr, m, v))
            g = gr * c
            m2 = b1 * m + omb1 * g
            v2 = b2 * v + (omb2 * g) * g
            d = np.sqrt(v2) / sb + eps
            p2 = p - step * (m2 / d)
            assert p2.dtype == f32 and m2.dtype == f32 and v2.dtype == f32
            P.append(p2), M.append(m2), V.append(v2)
    return s, P, M, V, True


def float64_trajectory(params, grads_per_step, lr, beta1, beta2, eps, max_grad_norm=None):
    """clip_grad_norm_ + Adam in float64 from float32 start values under a given gradient stream, with an exactly rounded norm.
    Yields per step what TrajectoryBound.step takes: (clipped grads, [(m, v) before], [(m, v) after], params after, sqrt(bc2),
    step_size)."""
    import math
    P = [np.asarray(p, f64).copy() for p in params]
    M, V = [np.zeros(p.shape, f64) for p in P], [np.zeros(p.shape, f64) for p in P]
    for t, G in enumerate(grads_per_step, 1):
        G = [np.asarray(g, f64) for g in G]
        norm = math.sqrt(math.fsum(float(x) * float(x) for g in G for x in g.reshape(-1)))
        coef = min(1.0, max_grad_norm / (norm + 1e-6)) if max_grad_norm else 1.0
        G = [g * coef for g in G]
        before = [(m.copy(), v.copy()) for m, v in zip(M, V)]
        bc1, bc2 = 1.0 - beta1 ** t, 1.0 - beta2 ** t
        M = [beta1 * m + (1.0 - beta1) * g for m, g in zip(M, G)]
        V = [beta2 * v + (1.0 - beta2) * g * g for v, g in zip(V, G)]
        P = [p - (lr / bc1) * (m / (np.sqrt(v) / math.sqrt(bc2) + eps)) for p, m, v in zip(P, M, V)]
        yield G, before, list(zip(M, V)), [p.copy() for p in P], math.sqrt(bc2), lr / bc1


# ------------------------------------------------------------------------------------------------------------------- the bound
class TrajectoryBound:
    """A first-order bound, element by element, on |float32 trajectory - float64 trajectory| of Adam under the SAME gradient
    stream, built from the float64 trajectory's own magnitudes and the float32 roundings the header's update makes (u = 2^-24;
    profiles/device_adam.md walks through it).  Per step, with e_m, e_v, e_p the bounds carried over:
      g~ = grad * coef            2 u |g|    (coef's conversion, the product)  + g_rel |g|  (a caller's extra term: a norm that
                                             is not the float64 one)
      m' = b1 m + (1 - b1) g~     e_m' = b1 e_m + 2 u |b1 m| + (2 u + r_g) |(1 - b1) g| + u |m'|
      v' = b2 v + ((1-b2) g~) g~  e_v' = b2 e_v + 2 u |b2 v| + (3 u + 2 r_g) |(1 - b2) g^2| + u |v'|
      s  = sqrt(v')               e_s  = min(e_v' / s, sqrt(e_v')) + u s
      q  = s / sqrt(bc2)          e_q  = e_s / sqrt(bc2) + 2 u q
      d  = q + eps                e_d  = e_q + u eps + u d
      r  = m' / d                 e_r  = e_m' / d + |m'| e_d / d^2 + u |r|
      p' = p - step_size r        e_p' = e_p + step_size e_r + 2 u |step_size r| + u |p'|
    where r_g = 2 u + g_rel.  Second-order terms and the float64 side's own roundings (1e-9 of these) are covered by the factor
    1.001."""

    def __init__(self, shapes, g_rel=0.0):
        self.em = [np.zeros(s, f64) for s in shapes]
        self.ev = [np.zeros(s, f64) for s in shapes]
        self.ep = [np.zeros(s, f64) for s in shapes]
        self.g_rel, self.u = g_rel, U32

    def step(self, k, g, m, v, m2, v2, p2, beta1, beta2, eps, bc2_sqrt, step_size):
        """Tensor k, all float64: the clipped gradient g (grad * coef), the moments before (m, v) and after (m2, v2) and the
        parameter after (p2) in the float64 trajectory.  -> e_p'."""
        u = self.u
        rg = 2 * u + self.g_rel
        g, m, v, m2, v2, p2 = (np.abs(np.asarray(x, f64)) for x in (g, m, v, m2, v2, p2))
        em = beta1 * self.em[k] + 2 * u * beta1 * m + (2 * u + rg) * (1 - beta1) * g + u * m2
        ev = beta2 * self.ev[k] + 2 * u * beta2 * v + (3 * u + 2 * rg) * (1 - beta2) * g * g + u * v2
        s = np.sqrt(v2)
        with np.errstate(all="ignore"):
            es = np.where(s > 0, np.minimum(ev / np.where(s > 0, s, 1.0), np.sqrt(ev)), np.sqrt(ev)) + u * s
        q = s / bc2_sqrt
        eq = es / bc2_sqrt + 2 * u * q
        d = q + eps
        ed = eq + u * eps + u * d
        r = m2 / d
        er = em / d + m2 * ed / (d * d) + u * r
        ep = self.ep[k] + step_size * er + 2 * u * step_size * r + u * p2
        self.em[k], self.ev[k], self.ep[k] = em * 1.001, ev * 1.001, ep * 1.001
        return self.ep[k]


def torch_norm_rel(total_numel):
    """A float32 norm of N elements in an order that is not ours: each of the N - 1 additions rounds once, the squares and the
    square root once each; the norm's relative error is half the sum's plus its own.  First order, in units of 1."""
    return (0.5 * (total_numel + 1) + 1) * U32


# ---------------------------------------------------------------------------------------------------------------------- cases
def gen_grad(kind, n, seed):
    r = np.random.default_rng([n, seed, 131])
    if kind == "normal":
        return r.standard_normal(n).astype(f32)
    if kind == "small":       # a norm far below any max_grad_norm
        return (r.standard_normal(n) * 1e-4).astype(f32)
    if kind == "large":
        return (r.standard_normal(n) * 30).astype(f32)
    if kind == "zero":
        return np.zeros(n, f32)
    if kind == "subnormal":   # float32 subnormals (below 1.18e-38), both signs, and a few zeros
        x = (r.integers(0, 1 << 20, n).astype(np.uint32) | (r.integers(0, 2, n).astype(np.uint32) << 31)).view(f32)
        return x.copy()
    raise ValueError(kind)


def gen_tensors(sizes, seed, kind="normal"):
    """-> params, grads, exp_avgs (any sign), exp_avg_sqs (>= 0): float32 lists, as after some training"""
    r = np.random.default_rng([len(sizes), seed, 977])
    P = [r.standard_normal(n).astype(f32) for n in sizes]
    G = [gen_grad(kind, n, seed + 17 * k) for k, n in enumerate(sizes)]
    M = [(r.standard_normal(n) * 0.1).astype(f32) for n in sizes]
    V = [(r.standard_normal(n) ** 2 * 0.01).astype(f32) for n in sizes]
    return P, G, M, V
