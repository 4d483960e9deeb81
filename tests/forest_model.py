"""Exact marginals on cycle-free Tanner graphs: a reference for flooding BP that
owes nothing to the oracle or to the kernels (no HIP, no oracle import).

On a forest, the belief of variable j after iteration t is the posterior
log-ratio of e_j in the model that keeps every prior and only the checks within
graph distance 2 t - 1 of j.  Here that posterior is computed by enumerating all
2^k error patterns of j's component: no messages, no schedule, no leave-one-out
passes.  Product-sum is the log-ratio of the two summed weights; min-sum with
ms_scaling = 1 is the difference of the two minimum costs, with
cost(e) = sum_i e_i log((1 - p_i) / p_i).  A variable that the kept checks
determine has belief +-inf: only its sign is defined.

A forest is a disjoint union of copies of small tree templates with its rows and
columns shuffled, so graphs of any size stay enumerable: the work is vectorised
over the copies of a template, and shots enter only through which patterns
satisfy the kept checks.  Everything is generated from seeds."""
import numpy as np
import scipy.sparse as sp

LD = np.longdouble
METHODS = ("ps", "ms")


class Template:
    """A tree grown from variable 0: step (v, r) attaches a check to the
    existing variable v and gives it r new variables.  No step: one isolated
    variable.  prior: the (lo, hi) range of its variables' priors, where the
    forest's own range would let the beliefs of a high-degree variable grow
    beyond what f32 probability ratios resolve (see settle).  hot: its
    variables may draw a prior above 0.5."""

    def __init__(self, name, steps, prior=None, hot=False):
        self.prior, self.hot = prior, hot
        rows, k = [], 1
        for v, r in steps:
            assert 0 <= v < k
            rows.append([v] + list(range(k, k + r)))
            k += r
        self.name, self.k, self.c, self.rows = name, k, len(rows), rows
        self.A = np.zeros((self.c, k), np.uint8)
        for i, r in enumerate(rows):
            self.A[i, r] = 1
        self.row_deg = self.A.sum(axis=1).astype(int)
        self.col_deg = self.A.sum(axis=0).astype(int)
        # dist[j, i]: graph distance from variable j to check i (odd), by BFS
        self.dist = np.full((k, self.c), -1, int)
        for j in range(k):
            seen_v, seen_c, front, d = {j}, set(), [j], 0
            while front:
                d += 1
                checks = [i for v in front for i in np.flatnonzero(self.A[:, v]) if i not in seen_c]
                for i in checks:
                    if i not in seen_c:
                        seen_c.add(i)
                        self.dist[j, i] = d
                d += 1
                front = []
                for i in checks:
                    for v in np.flatnonzero(self.A[i]):
                        if v not in seen_v:
                            seen_v.add(v)
                            front.append(v)
        assert (self.dist > 0).all(), "a template is one component"
        # iterations until every variable sees the whole component
        self.radius = int((self.dist.max() + 2) // 2) if self.c else 0
        self._pat = None

    def patterns(self):
        """(P, par): all 2^k patterns as bits, and their check parities."""
        if self._pat is None:
            P = ((np.arange(1 << self.k)[:, None] >> np.arange(self.k)) & 1).astype(np.uint8)
            self._pat = P, (P @ self.A.T) & 1
        return self._pat

    def check_sets(self, T, radius):
        """{tuple of kept checks: [(j, t), ...]} for t = 1..T."""
        out = {}
        for j in range(self.k):
            for t in range(1, T + 1):
                S = tuple(np.flatnonzero(self.dist[j] <= radius(t)).tolist())
                out.setdefault(S, []).append((j, t))
        return out


def template_beliefs(tpl, priors, syn, T, radius=lambda t: 2 * t - 1, use_syndrome=True):
    """{method: float64 [K, B, T, k]}: the exact belief of every variable of K
    copies of tpl (priors [K, k]) after iterations 1..T, for B shots per copy
    (syn uint8 [K, B, c]).  radius and use_syndrome exist for the mutation tests."""
    K, B = syn.shape[:2]
    k = tpl.k
    P, par = tpl.patterns()
    out = {me: np.empty((K, B, T, k)) for me in METHODS}
    if not use_syndrome:
        syn = np.zeros_like(syn)
    sets = tpl.check_sets(T, radius)
    step = max(1, (1 << 21) >> k)
    with np.errstate(divide="ignore", invalid="ignore"):
        for lo in range(0, K, step):
            p = priors[lo:lo + step].astype(LD)
            l1, l0 = np.log(p), np.log1p(-p)
            Pl = P.astype(LD)
            w = np.exp(l0.sum(axis=1)[:, None] + (l1 - l0) @ Pl.T)   # [Kc, 2^k] pattern weights
            cost = (l0 - l1) @ Pl.T                                   # [Kc, 2^k] pattern costs
            for S, users in sets.items():
                S = list(S)
                sig = par[:, S].astype(np.int64) @ (1 << np.arange(len(S), dtype=np.int64))
                order = np.argsort(sig, kind="stable")
                usig, starts = np.unique(sig[order], return_index=True)
                shot = syn[lo:lo + step][:, :, S].astype(np.int64) @ (1 << np.arange(len(S), dtype=np.int64))
                idx = np.searchsorted(usig, shot)                     # [Kc, B]
                assert (usig[np.minimum(idx, len(usig) - 1)] == shot).all(), "a syndrome no pattern gives"
                ws, cs = w[:, order], cost[:, order]
                by_j = {}
                for j, t in users:
                    by_j.setdefault(j, []).append(t)
                for j, ts in sorted(by_j.items()):
                    bit = P[order, j].astype(bool)[None, :]
                    z1 = np.add.reduceat(np.where(bit, ws, 0), starts, axis=1)
                    z0 = np.add.reduceat(np.where(bit, 0, ws), starts, axis=1)
                    m1 = np.minimum.reduceat(np.where(bit, cs, np.inf), starts, axis=1)
                    m0 = np.minimum.reduceat(np.where(bit, np.inf, cs), starts, axis=1)
                    ps = np.take_along_axis(np.log(z0) - np.log(z1), idx, axis=1)
                    ms = np.take_along_axis(m1 - m0, idx, axis=1)
                    for t in ts:
                        out["ps"][lo:lo + step, :, t - 1, j] = ps
                        out["ms"][lo:lo + step, :, t - 1, j] = ms
    return out


class Forest:
    """Copies of templates as one check matrix with shuffled rows and columns.

    parts: [(Template, copies)].  var_of[i] int [K, k] and chk_of[i] int [K, c]
    map the copies of parts[i] to columns and rows of H.  Priors are uniform in
    (lo, hi), or in the template's own range; a share hot of the columns of the
    templates that allow it gets a prior in (0.52, 0.7) instead.  (Product-sum
    decides bit by bit: a prior above 0.5 next to a check of degree 3 or more
    can leave a component whose decisions never satisfy it, and one such
    component keeps every shot of the graph from converging.)"""

    def __init__(self, parts, seed, lo, hi, hot=0.15):
        rng = np.random.default_rng(seed)
        self.parts = [(t, K) for t, K in parts if K > 0]
        self.n = sum(t.k * K for t, K in self.parts)
        self.m = sum(t.c * K for t, K in self.parts)
        cperm, rperm = rng.permutation(self.n), rng.permutation(self.m)
        self.var_of, self.chk_of, v0, c0 = [], [], 0, 0
        ri, ci = [], []
        for t, K in self.parts:
            vo = cperm[v0:v0 + t.k * K].reshape(K, t.k)
            co = rperm[c0:c0 + t.c * K].reshape(K, t.c)
            v0, c0 = v0 + t.k * K, c0 + t.c * K
            self.var_of.append(vo)
            self.chk_of.append(co)
            for i, r in enumerate(t.rows):
                ri.append(np.repeat(co[:, i], len(r)))
                ci.append(vo[:, r].ravel())
        ri = np.concatenate(ri) if ri else np.zeros(0, int)
        ci = np.concatenate(ci) if ci else np.zeros(0, int)
        self.H = sp.csr_matrix((np.ones(len(ri), np.uint8), (ri, ci)), shape=(self.m, self.n))
        self.H.sort_indices()
        self.lo, self.hi, self.hot = lo, hi, hot
        self.probs = np.empty(self.n)
        for (t, K), vo in zip(self.parts, self.var_of):
            self.probs[vo] = self.draw_priors(rng, t, vo.shape)
        self.logicals = (rng.random((3, self.n)) < 0.05).astype(np.uint8)

    def draw_priors(self, rng, tpl, size):
        p = rng.uniform(*(tpl.prior or (self.lo, self.hi)), size)
        hot = (rng.random(size) < self.hot) & tpl.hot
        return np.where(hot, rng.uniform(0.52, 0.7, size), p)

    def syndrome(self, e):
        return np.ascontiguousarray((self.H @ e.T).T % 2).astype(np.uint8)

    def beliefs(self, e, T, part=None, rows=None, **mut):
        """Per part (or the one asked for, on the copies rows): {method: [K, B, T, k]}
        for the shots whose errors are e uint8 [B, n]."""
        syn = self.syndrome(e)
        out = []
        for i, (t, K) in enumerate(self.parts):
            if part is not None and i != part:
                continue
            sel = slice(None) if rows is None else rows
            s = syn[:, self.chk_of[i][sel]].transpose(1, 0, 2)     # [K, B, c]
            out.append(template_beliefs(t, self.probs[self.var_of[i][sel]], s, T, **mut))
        return out

    def decode(self, e, T, **mut):
        """The model's decode of the shots with errors e: {method: dict(x, llr,
        iters, status, llr_t [B, T, n], flip [B], deep [B])}.  x_t = (belief <= 0);
        iters is the first t with H x_t = s, else T; x and llr are those of that
        iteration; status has bit 0 for a t found and bit 1 for H x = s.  flip: a decision changed between iteration
        iters - 1 and iters; deep: the largest radius among the components with a
        non-zero syndrome."""
        B = e.shape[0]
        syn = self.syndrome(e)
        per_part = self.beliefs(e, T, **mut)
        deep = np.zeros(B, int)
        for i, (t, K) in enumerate(self.parts):
            if t.c:
                hit = syn[:, self.chk_of[i]].any(axis=2)               # [B, K]
                deep = np.maximum(deep, hit.any(axis=1) * t.radius)
        out = {}
        for me in METHODS:
            llr_t = np.empty((B, T, self.n))
            for i, bel in enumerate(per_part):
                llr_t[:, :, self.var_of[i]] = bel[me].transpose(1, 2, 0, 3)
            x_t = (llr_t <= 0).astype(np.uint8)
            ok = np.empty((B, T), bool)
            for t in range(T):
                ok[:, t] = (self.syndrome(x_t[:, t]) == syn).all(axis=1)
            conv = ok.any(axis=1)
            iters = np.where(conv, ok.argmax(axis=1) + 1, T).astype(np.int32)
            at = iters - 1
            rows = np.arange(B)
            flip = np.array([at[b] > 0 and (x_t[b, at[b]] != x_t[b, at[b] - 1]).any() for b in range(B)])
            sat = ok[rows, at]
            out[me] = dict(x=x_t[rows, at], llr=llr_t[rows, at], iters=iters, status=(conv + 2 * sat).astype(np.uint8),
                           llr_t=llr_t, flip=flip, deep=deep)
        return out


def sample_errors(forest, rates, B, seed):
    """(e uint8 [B, n], rate [B]): shot b draws its error at rates[b % len(rates)]."""
    rng = np.random.default_rng(seed)
    rate = np.asarray(rates, float)[np.arange(B) % len(rates)]
    return (rng.random((B, forest.n)) < rate[:, None]).astype(np.uint8), rate


def settle(forest, e, rate, T, guard, cap, seed, rounds=40):
    """Redraw, in a seeded loop, the error of every (component, shot) that holds
    a belief with a magnitude below guard, or a finite one above cap, at some
    iteration under either method; from the fifth round on also the component's
    priors.  Changes e and forest.probs in place and returns the number of
    redraws; afterwards every finite belief of the shots lies within the two.

    guard keeps the rounding of a kernel from deciding a bit.  cap is about the
    number format of ldpc v1's product-sum, which works on probability ratios:
    a message of log-ratio L enters a check as 2 / (1 + exp(-|L|)) - 1, whose
    distance from 1 carries a relative error of exp(|L|) * 2^-24 in f32 and
    is lost altogether beyond |L| = 16.6.  Beliefs beyond cap would measure that
    format, not belief propagation."""
    rng = np.random.default_rng(seed)
    redraws = 0
    for i, (t, K) in enumerate(forest.parts):
        rows = np.arange(K)
        for rnd in range(rounds):
            bel = forest.beliefs(e, T, part=i, rows=rows)[0]
            bad = np.zeros(bel["ps"].shape[:2], bool)
            for me in METHODS:
                a = np.abs(bel[me])
                bad |= ((a < guard) | (np.isfinite(a) & (a > cap))).any(axis=(2, 3))
            if not bad.any():
                break
            kk, bb = np.nonzero(bad)
            redraws += len(kk)
            if rnd >= 4:
                for c in np.unique(kk):
                    forest.probs[forest.var_of[i][rows[c]]] = forest.draw_priors(rng, t, t.k)
            for c, b in zip(kk, bb):
                e[b, forest.var_of[i][rows[c]]] = rng.random(t.k) < rate[b]
            rows = rows[np.unique(kk)]
        else:
            raise AssertionError(f"beliefs below the guard remain in template {t.name}")
    return redraws
