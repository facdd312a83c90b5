"""Rule C17l restated: gated BS.1770 loudness of a 24 kHz mono f32 recording and the gain to a target, in numpy f64 with every product
and sum rounded once (ordinary operators: numpy never contracts).  x: n finite samples, |x| < 65520, each converted to f64 exactly.
    constants: the seven K-weighting coefficients at 24 kHz and the absolute gate A = 10^((-70 + 0.691) / 10), formed in double from the analog prototypes
        (formulas(fs), abs_gate_ms()); the tests pass the library's own values (bark_hip_loudness_constants) to everything below
    HOP = 2400, PRE = 4800, Hn = n // HOP; hop h: one run from zero state at sample max(0, (h - 2) HOP) to behind sample (h + 1) HOP - 1, each biquad in
        transposed direct form II, shelf then high-pass:  y = b0 x + s1;  s1 = (b1 x - a1 y) + s2;  s2 = b2 x - a2 y
        z[h] = the sum z + y2 y2 from +0 over the hop's own 2400 outputs, ascending
    blocks: J = Hn - 3 (none below 4 hops), S[j] = ((z[j] + z[j+1]) + z[j+2]) + z[j+3]
    gates (strict): absolute S[j] > 9600 A -> c1, sum1 (ascending);  relative S[j] c1 > 0.1 sum1 -> c2, sum2;  M = sum2 / (9600 c2)
    gain: J == 0 or c2 == 0 -> 1 exactly, flag UNMEASURABLE; else g = sqrt(Tms / M), min with max_gain (if > 0), min with ceiling / peak (both > 0);
        g32 = f32(g);  y[i] = x[i] g32, one f32 product
The hop runs are vectorised over (recording, hop) lanes: a loop of 7200 steps of elementwise operations.  A lane whose run starts at sample 0 (h < 2) is held
at zero state until its first sample."""
import math

import numpy as np

HOP, PRE, BLOCK_HOPS = 2400, 4800, 4
RUN = PRE + HOP
MAX_SAMPLES = 4096 * 320
MAX_ABS = 65520.0
T_MIN, T_MAX = -4000, -500
UNMEASURABLE, CAP_BOUND, CEILING_BOUND = 1, 2, 4
ITU_48K = dict(shelf_b=(1.53512485958697, -2.69169618940638, 1.19839281085285), shelf_a=(-1.69065929318241, 0.73248077421585),
               hp_b=(1.0, -2.0, 1.0), hp_a=(-1.99004745483398, 0.99007225036621))


def formulas(fs: float = 24000.0) -> np.ndarray:
    """[shelf b0, b1, b2, a1, a2, high-pass a1, a2] at the rate fs, in double"""
    G, Q, fc = 3.999843853973347, 0.7071752369554196, 1681.974450955533
    K = math.tan(math.pi * fc / fs)
    Vh = 10.0 ** (G / 20.0)
    Vb = Vh ** 0.4996667741545416
    a0 = 1.0 + K / Q + K * K
    out = [(Vh + Vb * K / Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0]
    Q, fc = 0.5003270373238773, 38.13547087602444
    K = math.tan(math.pi * fc / fs)
    a0 = 1.0 + K / Q + K * K
    out += [2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0]
    return np.asarray(out, np.float64)


def abs_gate_ms() -> float:
    return 10.0 ** ((-70.0 + 0.691) / 10.0)


def constants() -> np.ndarray:
    """what bark_hip_loudness_constants hands out: the seven coefficients, A, 9600 A"""
    a = abs_gate_ms()
    return np.concatenate([formulas(24000.0), [a, 9600.0 * a]])


def target_ms(centilufs: int) -> float:
    return 10.0 ** ((centilufs / 100.0 + 0.691) / 10.0)


def lufs_of(ms: float) -> float:
    return -0.691 + 10.0 * math.log10(ms) if ms > 0.0 else -math.inf


def hops(xs, k=None) -> list:
    """the z table of every recording of xs: one f64 array of Hn values each"""
    k = constants() if k is None else np.asarray(k, np.float64)
    b0, b1, b2, a1, a2, ha1, ha2 = (np.float64(v) for v in k[:7])
    xs = [np.ascontiguousarray(x, np.float32).reshape(-1) for x in xs]
    lanes = [(r, h) for r, x in enumerate(xs) for h in range(len(x) // HOP)]
    out = [np.zeros(len(x) // HOP, np.float64) for x in xs]
    if not lanes:
        return out
    L = len(lanes)
    first = np.asarray([(h - 2) * HOP for _, h in lanes])                       # sample index of step 0; below 0: the run has not begun
    steps = np.zeros((RUN, L), np.float64)                                      # steps[i][lane]: the sample of step i, f32 -> f64 exactly
    for lane, (r, h) in enumerate(lanes):
        lo = max(0, (h - 2) * HOP)
        steps[RUN - ((h + 1) * HOP - lo):, lane] = xs[r][lo:(h + 1) * HOP].astype(np.float64)
    s1 = np.zeros(L); s2 = np.zeros(L); t1 = np.zeros(L); t2 = np.zeros(L); z = np.zeros(L)
    for i in range(RUN):
        x = steps[i]
        y = b0 * x + s1
        s1 = (b1 * x - a1 * y) + s2
        s2 = b2 * x - a2 * y
        y2 = y + t1                                                             # high-pass b = 1, -2, 1: 1 y is y
        t1 = (-2.0 * y - ha1 * y2) + t2
        t2 = y - ha2 * y2
        before = first + i < 0                                                  # the run starts from zero state at sample 0
        if before.any():
            s1[before] = 0.0; s2[before] = 0.0; t1[before] = 0.0; t2[before] = 0.0
        if i >= PRE:
            z = z + y2 * y2
    for lane, (r, h) in enumerate(lanes):
        out[r][h] = z[lane]
    return out


def gates(z, k=None):
    """(M, J, c1, c2) of one recording's z table; M is 0.0 where nothing passes"""
    k = constants() if k is None else np.asarray(k, np.float64)
    gate = np.float64(k[8])
    z = np.asarray(z, np.float64)
    J = len(z) - 3 if len(z) >= BLOCK_HOPS else 0
    S = [((z[j] + z[j + 1]) + z[j + 2]) + z[j + 3] for j in range(J)]
    c1, sum1 = 0, np.float64(0.0)
    for s in S:
        if s > gate:
            c1 += 1; sum1 = sum1 + s
    c2, sum2 = 0, np.float64(0.0)
    rel = np.float64(0.1) * sum1
    for s in S:
        if s > gate and s * np.float64(c1) > rel:
            c2 += 1; sum2 = sum2 + s
    M = float(sum2 / (np.float64(9600.0) * np.float64(c2))) if c2 else 0.0
    return M, J, c1, c2


def measure(x, z=None, k=None) -> dict:
    x = np.ascontiguousarray(x, np.float32).reshape(-1)
    z = hops([x], k)[0] if z is None else z
    M, J, c1, c2 = gates(z, k)
    return dict(mean_square=M, lufs=lufs_of(M), peak=np.float32(np.max(np.abs(x))) if len(x) else np.float32(0.0), n_blocks=J, n_abs=c1, n_gated=c2,
                flags=UNMEASURABLE if c2 == 0 else 0, z=z)


def gain_of(info: dict, tms: float, peak_ceiling: float = 1.0, max_gain: float = 10.0):
    """(g32, flags) of a measured recording for the target mean square tms"""
    flags = info["flags"]
    if flags & UNMEASURABLE:
        return np.float32(1.0), flags
    g = np.sqrt(np.float64(tms) / np.float64(info["mean_square"]))
    if max_gain > 0 and np.float64(np.float32(max_gain)) < g:
        g = np.float64(np.float32(max_gain)); flags |= CAP_BOUND
    if peak_ceiling > 0 and info["peak"] > 0:
        lim = np.float64(np.float32(peak_ceiling)) / np.float64(info["peak"])
        if lim < g:
            g = lim; flags = (flags & ~CAP_BOUND) | CEILING_BOUND
    return np.float32(g), flags


def level(x, tms: float, peak_ceiling: float = 1.0, max_gain: float = 10.0, z=None, k=None):
    """(y, info) of one recording: info as measure() plus gain and the flags of the gain"""
    x = np.ascontiguousarray(x, np.float32).reshape(-1)
    info = measure(x, z, k)
    g32, flags = gain_of(info, tms, peak_ceiling, max_gain)
    info["gain"] = g32; info["flags"] = flags
    return x * g32, info


def level_many(xs, tms, peak_ceiling: float = 1.0, max_gain: float = 10.0, k=None) -> list:
    """level() of every recording, the hop runs of all of them in one vectorised pass; tms: one value or one per recording (0: off, gain 1)"""
    tms = [tms] * len(xs) if np.isscalar(tms) else list(tms)
    zs = hops(xs, k)
    out = []
    for x, t, z in zip(xs, tms, zs):
        if t == 0:
            info = measure(x, z, k); info["gain"] = np.float32(1.0)
            out.append((np.ascontiguousarray(x, np.float32).copy(), info))
        else:
            out.append(level(x, t, peak_ceiling, max_gain, z, k))
    return out
