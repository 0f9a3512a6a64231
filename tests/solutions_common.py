"""What the solution-set tests share (tests/test_solutions_emulation.py on the CPU, tests/test_gpu_solutions.py on the device): the greedy
rule of include/ikgpu.h (ikgpu_dls_solutions_batch) restated in numpy over the K single solves, and the three assertions that follow
from the definition."""
import numpy as np

NAN_FILL, INT_FILL = float("nan"), -7     # what the callers prefill the outputs with


def greedy(singles, support, sep, N):
    """singles[k] = (q [B, nq], success [B], iters [B]) of the single solve from start k; support [nq] bool.
    Returns (count [B], which [N, B] with INT_FILL in the unused slots, dropped [B]: converged starts refused as near-duplicates)."""
    K, B = len(singles), singles[0][0].shape[0]
    count, which, dropped = np.zeros(B, np.int32), np.full((N, B), INT_FILL, np.int32), np.zeros(B, np.int32)
    for b in range(B):
        kept = []
        for k in range(K):
            if not singles[k][1][b] or len(kept) >= N:
                continue
            qk = singles[k][0][b][support]
            # one IEEE subtraction, fabs and a compare per entry
            if all((np.abs(qk - singles[j][0][b][support]) >= sep).any() for j in kept):
                kept.append(k)
            else:
                dropped[b] += 1
        count[b] = len(kept)
        which[:len(kept), b] = kept
    return count, which, dropped


def check_set(got, singles, support, sep, N, label=""):
    """got = (Q [N, B, nq], count [B], which [N, B] or None, iters [N, B] or None), the outputs prefilled with NAN_FILL / INT_FILL."""
    Q, count, which, iters = got
    want_count, want_which, _ = greedy(singles, support, sep, N)
    # 1. count and which are the greedy rule's
    assert np.array_equal(count, want_count), (label, "count")
    if which is not None:
        assert np.array_equal(which, want_which), (label, "which")
    B = count.shape[0]
    qs = np.stack([s[0] for s in singles])       # [K, B, nq]
    its = np.stack([s[2] for s in singles])      # [K, B]
    rows = np.arange(B)
    for n in range(N):
        w = n < want_count
        # 2. every written slab is the single solve from which[n][b], over all nq entries
        src = np.where(w, want_which[n], 0)
        assert np.array_equal(Q[n][w], qs[src, rows][w]), (label, "q", n)
        if iters is not None:
            assert np.array_equal(iters[n][w], its[src, rows][w]), (label, "iterations", n)
            assert (iters[n][~w] == INT_FILL).all(), (label, "iterations of an unused slot", n)
        # 3. unwritten slots still hold their prefill
        assert np.isnan(Q[n][~w]).all(), (label, "q of an unused slot", n)
    return want_count, want_which
