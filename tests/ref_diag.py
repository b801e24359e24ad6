"""numpy restatement of the convergence diagnostics ("Convergence diagnostics"; csrc/ngp_diag.h): the streaming
lag-window autocovariance, the finalising step and the pooling over chains.  Elementwise fp64 over the D-vector: numpy does not
fuse, so every product and sum is rounded on its own, as the device rounds it (-ffp-contract=off)."""
import numpy as np


class Stream:
    """The state of one chain: x1[D] | S1[2][D] | S2[2][D] | C[L][D] | head[L][D] | ring[L][D], n draws taken, split H."""

    def __init__(self, D, lags=64, split=0):
        self.D, self.L, self.H, self.n = int(D), int(lags), int(split), 0
        self.x1 = np.zeros(D)
        self.S1, self.S2 = np.zeros((2, D)), np.zeros((2, D))
        self.C, self.head, self.ring = np.zeros((self.L, D)), np.zeros((self.L, D)), np.zeros((self.L, D))

    def update(self, x):
        t, L = self.n, self.L
        x = np.asarray(x, dtype=np.float64)
        if t == 0:
            self.x1 = x.copy()
        y = x - self.x1
        for k in range(1, min(t, L - 1) + 1):
            self.C[k] = self.C[k] + y * self.ring[(t - k) % L]
        h = 0 if t < self.H else 1
        self.S1[h] = self.S1[h] + y
        self.S2[h] = self.S2[h] + y * y
        if t < L:
            self.head[t] = y
        self.ring[t % L] = y
        self.n += 1

    def image(self):
        return np.concatenate([self.x1, self.S1.ravel(), self.S2.ravel(), self.C.ravel(), self.head.ravel(), self.ring.ravel()])

    def finalise(self):
        n, L, D = self.n, self.L, self.D
        nan = np.full(D, np.nan)
        with np.errstate(all="ignore"):
            s1, s2 = self.S1[0] + self.S1[1], self.S2[0] + self.S2[1]
            m = s1 / float(n)
            g0 = s2 - m * s1
            var = g0 / float(n - 1) if n >= 2 else nan.copy()
            ess, trunc = np.full(D, float(n)), np.zeros(D)
            if n >= 4:
                K = min(L, n)
                mm = m * m
                hs, ts = np.zeros(D), np.zeros(D)
                tau, gprev = np.full(D, -1.0), g0.copy()
                live = g0 > 0.0            # still adding pairs
                hit = np.zeros(D, dtype=bool)
                for k in range(1, K):
                    hs = hs + self.head[k - 1]
                    ts = ts + self.ring[(n - k) % L]
                    gk = (self.C[k] - m * ((s1 - hs) + (s1 - ts))) + float(n - k) * mm
                    if k & 1:
                        pair = (gprev + gk) / g0
                        stop = live & ~(pair > 0.0)
                        hit |= stop
                        live &= ~stop
                        tau = np.where(live, tau + 2.0 * pair, tau)
                    else:
                        gprev = gk
                on = g0 > 0.0
                trunc = np.where(on & ~hit & (K < n), 1.0, 0.0)
                e = float(n) / np.where(tau > 1e-12, tau, 1e-12)
                ess = np.where(on, np.where(e < float(n), e, float(n)), float(n))
            mean = m + self.x1
            mcse = np.sqrt(var / ess)
            n0 = min(n, self.H)
            half_n = np.array([float(n0), float(n - n0)])
            half_mean, half_var = np.empty((2, D)), np.empty((2, D))
            for h, nh in enumerate((n0, n - n0)):
                mh = self.S1[h] / float(nh)
                half_mean[h] = mh + self.x1 if nh >= 1 else nan
                half_var[h] = (self.S2[h] - mh * self.S1[h]) / float(nh - 1) if nh >= 2 else nan
        return dict(n=n, mean=mean, var=var, sd=np.sqrt(var), ess=ess, mcse=mcse, truncated=trunc, half_n=half_n, half_mean=half_mean, half_var=half_var)


def sample_theta(S):
    """The monitored vector of every record of a sample file, [n, D], from read_sample_file's dict: varE | b | b_fixed | u of every
    random-effect set, then varU | beta | varBeta | piHat | class probabilities | thr (models without BayesLV sets)."""
    assert not S["lv_c"], "BayesLV words: not restated here"
    parts = [S["varE"][:, None], S["b"][:, None], S["b_fixed"]] + list(S["u"]) + [S["varU"], S["beta"], S["varBeta"], S["piHat"], S["class_pi"]]
    if "thr" in S:
        parts.append(S["thr"])
    return np.concatenate([np.asarray(p, dtype=np.float64) for p in parts], axis=1)


def run(theta, lags=64, split=0):
    """The stream over the rows of theta [n, D]."""
    theta = np.atleast_2d(np.asarray(theta, dtype=np.float64))
    s = Stream(theta.shape[1], lags, split)
    for x in theta:
        s.update(x)
    return s


def pool(per_chain):
    """Split-R-hat and pooled summaries of the chains' finalised diagnostics: the sequences are every half with n_s >= 2 of every chain."""
    D = len(per_chain[0]["mean"])
    seq_n, seq_mean, seq_var = [], [], []
    for c in per_chain:
        for h in range(2):
            if c["half_n"][h] >= 2:
                seq_n.append(float(c["half_n"][h])); seq_mean.append(c["half_mean"][h]); seq_var.append(c["half_var"][h])
    ns = np.array([float(c["n"]) for c in per_chain])
    with np.errstate(all="ignore"):
        mean = sum(n * c["mean"] for n, c in zip(ns, per_chain)) / ns.sum()
        ess = sum(c["ess"] for c in per_chain)
        if len(seq_n) >= 2:
            W = np.mean(seq_var, axis=0)
            n_bar = float(np.mean(seq_n))
            Bn = np.var(np.array(seq_mean), axis=0, ddof=1)
            vp = (n_bar - 1.0) / n_bar * W + Bn
            rhat = np.where(W > 0, np.sqrt(vp / W), np.nan)
        else:
            vp = np.mean(seq_var, axis=0) if seq_n else np.full(D, np.nan)
            rhat = np.full(D, np.nan)
        sd = np.sqrt(vp)
        return dict(n=int(ns.sum()), mean=mean, sd=sd, ess=ess, mcse=sd / np.sqrt(ess), rhat=rhat,
                    truncated=np.any([c["truncated"] > 0 for c in per_chain], axis=0).astype(np.float64))
