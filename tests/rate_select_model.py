"""numpy statement of kdlae_rate_select's rule (include/kdlae.h), shared by the CPU and GPU rate-sweep tests.

Per image b over scores[r][b]: mode 0 = argmin |score - target[b]| (fp32), 1 = argmax, 2 = argmin; ties go to
the lowest r; a NaN is never chosen; all NaN -> 0."""
import numpy as np

MODES = {"closest": 0, "max": 1, "min": 2}


def select_keys(scores, mode, target=None):
    s = np.asarray(scores, dtype=np.float32)
    if mode == 0:
        return np.abs(s - np.asarray(target, dtype=np.float32)[None, :]).astype(np.float32)
    return -s if mode == 1 else s


def select_model(scores, mode, target=None):
    """Vectorised: int32 [B]."""
    key = select_keys(scores, mode, target)
    valid = ~np.isnan(key)
    first_min = np.argmin(np.where(valid, key, np.inf), axis=0)      # first occurrence of the least valid key
    cols = np.arange(key.shape[1])
    # a column whose argmin landed on a NaN has only +inf keys among its valid ones (or none): first valid, else 0
    first_valid = np.argmax(valid, axis=0)
    return np.where(valid[first_min, cols], first_min, first_valid).astype(np.int32)


def select_loop(scores, mode, target=None):
    """The rule spelled out one score at a time."""
    s = np.asarray(scores, dtype=np.float32)
    R, B = s.shape
    out = np.zeros(B, dtype=np.int32)
    for b in range(B):
        best, bk = -1, None
        for r in range(R):
            v = s[r, b]
            if mode == 0:
                k = np.float32(abs(np.float32(v - np.float32(target[b]))))
            else:
                k = -v if mode == 1 else v
            if k != k:
                continue
            if best < 0 or k < bk:
                best, bk = r, k
        out[b] = max(best, 0)
    return out


def select_cases(R, B, seed=0):
    """(name, scores f32 [R,B], target f32 [B]) with planted ties, NaNs, signed zeros and midway targets."""
    rng = np.random.default_rng(1000 * R + 10 * B + seed)
    cases = []
    tgt = rng.uniform(-1, 1, B).astype(np.float32)
    cases.append(("random", rng.uniform(-1, 1, (R, B)).astype(np.float32), tgt))
    # few distinct values: ties everywhere, +0 / -0 among them
    vals = np.array([-0.5, -0.0, 0.0, 0.25, 0.75, 0.75], dtype=np.float32)
    cases.append(("ties", vals[rng.integers(0, len(vals), (R, B))], np.full(B, 0.5, np.float32)))
    cases.append(("signed-zero", np.where(rng.integers(0, 2, (R, B)) == 1, np.float32(0.0), np.float32(-0.0))
                  .astype(np.float32), np.zeros(B, np.float32)))
    s = rng.uniform(-1, 1, (R, B)).astype(np.float32)
    s[rng.integers(0, R), rng.integers(0, B)] = np.nan              # one NaN
    s[:, B - 1] = np.nan                                            # a column of all NaN
    cases.append(("nan", s, tgt))
    s = rng.uniform(-1, 1, (R, B)).astype(np.float32)
    s[0, :] = np.nan                                                # the first candidate is never eligible
    if R > 1:
        s[R - 1, 0] = np.inf
        s[1:R - 1, 0] = np.nan                                      # column 0: NaN .. NaN, +inf
    cases.append(("nan-first-inf-last", s, tgt))
    # target exactly midway between the two nearest scores: |0.25 - 0.5| == |0.75 - 0.5| in fp32
    s = np.full((R, B), 3.0, np.float32)
    s[R - 1, :] = 0.25
    s[R // 2, :] = 0.75
    cases.append(("midway", s, np.full(B, 0.5, np.float32)))
    return cases
