"""What the multi-start tests share (tests/test_multistart_emulation.py on the CPU, tests/test_gpu_multistart.py on the device): the
workload and the assertions that follow from the definition in include/ikgpu.h (ikgpu_dls_multistart_batch).

Workload: targets are the task frame's placement at configurations drawn uniformly between the joint limits, starts are drawn the same
way (np.random.default_rng(seed)) -- the regime in which a single start of ik::dls converges for 36-41 % of the problems on an arm."""
import numpy as np

MASK64 = (1 << 64) - 1


def uniform_configurations(model, B, seed):
    """(start [B, nq], configuration whose forward kinematics is the target [B, nq])."""
    lo, hi = np.asarray(model.lowerPositionLimit), np.asarray(model.upperPositionLimit)
    assert np.isfinite(lo).all() and np.isfinite(hi).all()
    rng = np.random.default_rng(seed)
    qt = rng.uniform(lo, hi, size=(B, model.nq))
    q0 = rng.uniform(lo, hi, size=(B, model.nq))
    return q0, qt


def mix(z):
    z &= MASK64
    z ^= z >> 30
    z = (z * 0xBF58476D1CE4E5B9) & MASK64
    z ^= z >> 27
    z = (z * 0x94D049BB133111EB) & MASK64
    z ^= z >> 31
    return z


def uniform(seed, b, k, i):
    """u of (seed, b, k, i): the formula of include/ikgpu.h restated."""
    h = mix(seed + 0x9E3779B97F4A7C15)
    h = mix(h + b)
    h = mix(h + k)
    h = mix(h + i)
    return (h >> 11) * 2.0 ** -53


def draw(seed, b, k, i, lo, hi):
    from fractions import Fraction
    v = float(Fraction(uniform(seed, b, k, i)) * Fraction(hi - lo) + Fraction(lo))   # one rounding, as the fused multiply-add
    return min(max(v, lo), hi)


def check_selection(got, singles, errs, err_at_result, label=""):
    """got = (q [B, nq], success [B], iters [B], winner [B], err_sq [B]) of the multi-start call; singles[k] = (q, success, iters) of the
    single solve from start k; errs[k] [B] = ||e||^2 of the reference evaluation at singles[k]'s q; err_at_result [B] = ||e|| of the
    reference evaluation at got's q.  The three assertions of the definition."""
    q, ok, it, win, err_sq = got
    B, K = q.shape[0], len(singles)
    assert win.min() >= 0 and win.max() < K, label
    rows = np.arange(B)
    # 1. the outputs are the single solve's from start winner[b], bit for bit
    for x, ref, what in zip((q, ok, it), zip(*singles), ("q", "success", "iterations")):
        assert np.array_equal(x, np.stack(ref)[win, rows]), (label, what)
    # 2. the winner has the minimal key: exact in the success class and in the index among successes ...
    S = np.stack([s[1] for s in singles]).astype(bool)      # [K, B]
    any_ok = S.any(axis=0)
    first_ok = S.argmax(axis=0)
    assert np.array_equal(ok.astype(bool), any_ok), label
    assert np.array_equal(win[any_ok], first_ok[any_ok]), label
    # ... and among failures the smallest error, to 1e-10 in the norm
    E = np.sqrt(np.stack(errs))                             # [K, B]
    fail = ~any_ok
    assert (E[win, rows][fail][None, :] <= E[:, fail] + 1e-10).all(), label
    # 3. err_sq is the winner's error
    assert np.isfinite(err_sq).all() and (err_sq >= 0).all(), label
    worst = float(np.abs(np.sqrt(err_sq) - err_at_result).max())
    assert worst <= 5e-11, (label, worst)
    return worst
