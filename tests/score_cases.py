"""The seeded rows that tests/test_score.py (CPU) and tests/test_score_gpu.py score against tests/score_ref.py.  Small on
purpose: one row per way the row arithmetic or the kernel's lane split can go wrong.  groups() gives three sets of rows, one per
mask mode (a call has one mode); OPTION_SETS the two settings every set is scored under."""
import functools

import numpy as np

N = 4672
HUBER_DELTA = 0.5
OPTION_SETS = (dict(label_smoothing=0.0, value_loss="mse", huber_delta=1.0),
               dict(label_smoothing=0.05, value_loss="huber", huber_delta=HUBER_DELTA))


class _Rows:
    def __init__(self, seed, masked):
        self.rng = np.random.default_rng(seed)
        self.masked = masked
        self.names, self.logits, self.pi, self.mask, self.value, self.z = [], [], [], [], [], []

    def add(self, name, support, pi, logits=None, value=None):
        """support: columns of the legal mask (masked sets) -- pi: {column: weight}; logits: {column: value} over seeded noise"""
        k = len(self.names)
        row = (self.rng.standard_normal(N) * 2.0).astype(np.float32)
        for c, x in (logits or {}).items():
            row[c] = x
        p = np.zeros(N, np.float32)
        for c, w in pi.items():
            p[c] = w
        m = np.zeros(N, np.uint8)
        m[list(support)] = 1
        z = float((-1, 0, 1)[k % 3])
        # |v - z| on both sides of HUBER_DELTA
        v = z + (0.3, -0.8, -0.2, 0.9)[k % 4] if value is None else value
        self.names.append(name); self.logits.append(row); self.pi.append(p); self.mask.append(m)
        self.value.append(np.float32(v)); self.z.append(np.float32(z))

    def soft(self, cols):
        w = self.rng.dirichlet(np.full(len(cols), 0.3)).astype(np.float32) + np.float32(1e-6)
        return dict(zip(cols, (w / w.sum()).tolist()))

    def pick(self, n, lo=0, hi=N):
        return sorted(self.rng.choice(np.arange(lo, hi), size=n, replace=False).tolist())

    def done(self, name, mode):
        return dict(name=name, mask_mode=mode, names=self.names, logits=np.stack(self.logits), pi=np.stack(self.pi),
                    value=np.array(self.value, np.float32), z=np.array(self.z, np.float32),
                    mask=np.stack(self.mask) if self.masked else None)


def _common(r):
    """rows every mode gets; the support is the mask (masked sets) and carries pi (so it is the support under `target` too)"""
    c = r.pick(1)
    r.add("support of 1", c, {c[0]: 1.0})
    c = r.pick(218)
    r.add("support of 218, soft pi", c, r.soft(c))
    c = r.pick(20, 300, 4000)
    pi = r.soft(c)
    r.add("+3e4 after -3e4 inside the support, the target on +3e4", c, pi | {c[3]: 0.0, c[9]: 2.0 * max(pi.values())},
          logits={c[3]: -3e4, c[9]: 3e4})
    r.add("-3e4 after +3e4 inside the support, pi on both", c, pi, logits={c[2]: 3e4, c[15]: -3e4})
    c = [0] + r.pick(30, 1)
    r.add("best logit and target at column 0", c, r.soft(c) | {0: 0.9}, logits={0: 25.0})
    c = r.pick(30, 0, N - 1) + [N - 1]
    r.add("best logit and target at column 4671", c, r.soft(c) | {N - 1: 0.9}, logits={N - 1: 25.0})
    c = r.pick(12, N - 64)
    r.add("support only in the last 16 pieces", c, r.soft(c))
    c = sorted(256 * k + j for k in r.pick(6, 0, 19) for j in r.pick(2, 0, 4) if 256 * k + j < N)
    r.add("support only in lane 0's columns", c, r.soft(c))
    c = r.pick(25)
    r.add("equal logits at the target", c, r.soft(c) | {c[7]: 0.8}, logits={c[7]: 1.5, c[2]: 1.5, c[20]: 1.5, c[11]: 2.5})
    c = r.pick(25)
    pi = dict.fromkeys(c, 0.2 / 23)
    pi[c[4]] = pi[c[18]] = 0.4
    r.add("equal pi maxima, the lower index with the lower logit", c, pi, logits={c[4]: -1.0, c[18]: 3.0, c[9]: 1.0, c[10]: 0.0})


@functools.lru_cache(maxsize=None)
def groups():
    legal = _Rows(11, True)
    _common(legal)
    c = legal.pick(30)
    out = [x for x in legal.pick(40) if x not in c][0]
    legal.add("one-hot pi outside the legal mask", c, {out: 1.0})
    c = legal.pick(35)
    legal.add("legal moves without pi on most of them", c, legal.soft(c[:5]))
    c = legal.pick(31)
    legal.add("pi summing to 0 with a mask", c, {})
    legal.add("empty support", [], {})
    c = legal.pick(28)
    far = [x for x in legal.pick(40) if x not in c][0]
    legal.add("+3e4 and -3e4 outside the support", c, legal.soft(c), logits={far: 3e4, (far + 1) % N: -3e4})
    legal.add("a NaN logit outside the support", c, legal.soft(c), logits={far: np.nan})
    legal.add("an infinite value", c, legal.soft(c), value=np.inf)

    target = _Rows(12, False)
    _common(target)
    target.add("empty support", [], {})
    c = target.pick(9)
    target.add("a -inf logit outside the support", c, target.soft(c), logits={[x for x in range(N) if x not in c][5]: -np.inf})

    none = _Rows(13, False)
    for k, (col, lg) in enumerate([(0, 25.0), (N - 1, 25.0), (1234, -2.0), (4000, 0.5), (77, 3e4), (2900, 1.0)]):
        extra = {5: -3e4} if k == 4 else {1234 + 64: -2.0, 9: 3.0} if k == 2 else {}
        none.add(f"one-hot at {col}", [], {col: 1.0}, logits=extra | {col: lg})
    return legal.done("legal", "legal"), target.done("target", "target"), none.done("none", "none")


def tiled(g, B, shift=0):
    """the set's rows repeated cyclically up to B, starting at row `shift`: (logits, value, pi, z, mask), and the row numbers"""
    idx = (np.arange(B) + shift) % len(g["names"])
    take = lambda a: None if a is None else np.ascontiguousarray(a[idx])
    return (take(g["logits"]), take(g["value"]), take(g["pi"]), take(g["z"]), take(g["mask"])), idx
