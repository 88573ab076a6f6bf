"""Float64 references, derived tolerances and case lists shared by tests/test_corr_cases_cpu.py (the references against the torch restatements,
the peak margins of the planted cases) and tests/test_corr_shapes_gpu.py (the comparisons with the kernels of csrc/ring.hip and csrc/fft2d.hip).
No test functions here.  Every reference is written from the formulas in the headers of those two files, in NumPy float64 (np.fft or direct
sums), and is computed once per process and shared read-only (functools.lru_cache).

Tolerances of the hand-written direct-sum kernels (k_ring_corr, k_dft_angle_r2c, k_dft_row_mag, k_corr_spectra, k_solve_translation) are DERIVED,
not measured.  With u = 2^-24 (fp32 unit roundoff) a length-N chain acc = fma(a_j, b_j, acc) has forward error at most
gamma_N * sum_j |a_j b_j|, gamma_N = N u / (1 - N u) (Higham, Accuracy and Stability of Numerical Algorithms, section 3.1); to first order N u.

  k_ring_corr     one chain of length A per (shift n, column d, channel c): |err corr[n,d]| <= A u sum_j |x||y|.  | |a| - |b| | <= |a - b|, so the
                  same bound holds after the magnitude.  The sum over d (wave reduction: 6 additions; the part[] slots: 3), over c (C additions)
                  and the scaling by A^-1/2 (the constant and the product: 2) each add one rounding relative to a partial sum that is itself
                  at most sum |x||y|:  first-order bound (A + C + 12) u A^-1/2 sum_c sum_d sum_j |x[c,(j+n)%A,d]| |y[c,j,d]| per shift n.
  k_dft_angle_r2c, k_dft_row_mag
                  a chain of length N per output component, one rounding per stored twiddle, the scaling (2), and for the magnitude two
                  products, a sum and a square root (4, with slack 8 in all): (N + 8) u N^-1/2 sum_j |x_j| (|cos| + |sin|) on the complex error
                  (real and imaginary part added), which also bounds the error of the magnitude.
  k_corr_spectra  the product a * conj(b) (2 roundings per component, relative to |a.x b.x| + |a.y b.y| and its like), a chain of length A whose
                  terms carry 2 roundings of their own, the twiddle (1), the scaling (2), the magnitude (4), the sum over d (at most 4 + 6
                  additions) and over c (C): (A + C + 24) u A^-1/2 sum_c sum_d sum_k (|z.x| + |z.y|)(|cos| + |sin|), z the absolute-value form of
                  the product.
  k_solve_translation
                  a chain of length W per (row, lag, channel), the scaling (2) and the sum over channels (C):
                  (W + C + 4) u W^-1/2 sum_c sum_j |q||p| per lag.

Every `allow` returned here is TWICE the first-order bound (the factor covers the 1 / (1 - N u) of gamma_N and second-order terms with a wide
margin).  Derived outputs: dist = 1 - max / denom adds the rounding of denom, of the quotient and of the difference: allow_dist = max(allow) /
denom + 4 u max(1, max / denom).

The rocFFT-backed values (DiSCO signature / spectrum, phase correlation, BEV translation) have no derivable bound from this project's code: their
bar is measured, 4 x the error (relative L2, see rel_l2) of the torch fp32 CPU restatement (oracle/corr_oracle.py) against the same float64 reference
on the same input, and element by element never looser than the form the existing DiSCO / BEV tests use (FFT_FORMS).  A planted argmax holds exactly whenever the reference's top value leads
its second by more than 10 x the allowance; tests/test_corr_cases_cpu.py asserts that for every planted case, so that the GPU tests compare every
angle, shift and argmax with no "only if unambiguous" escape.
"""
import functools

import numpy as np

U = 2.0 ** -24

# ---------------------------------------------------------------------------------------------------------------------------- case lists
SWEEP_SHAPES = [(1, 30, 34), (2, 30, 34), (1, 60, 256), (1, 150, 100), (3, 90, 20), (1, 60, 64), (1, 120, 120)]        # (C, A, D); Q = 3, N = 6
# many candidates per workgroup: (C, A, D, Q, n_db as a function of the compute-unit count)
MANY = {"q1": (1, 30, 34, 1, lambda cu: 2 * cu + 37), "q5": (1, 30, 34, 5, lambda cu: 2 * cu + 37),
        "c2": (2, 30, 34, 1, lambda cu: 2 * cu + 37), "big": (1, 120, 120, 1, lambda cu: cu + 44)}
NOMINAL_CU = 256                       # the compute-unit count the CPU margin test assumes (MI355X); entry i does not depend on the count
TIE_SHAPES = [(1, 30, 34), (1, 120, 120)]
REJECTED = [(1, 45, 33), (1, 30, 33), (1, 30, 257), (1, 120, 256)]     # A odd; A*D % 4 != 0; D > 256; tiles exceed the LDS
DFT_SHAPES = [(120, 120), (30, 34), (45, 33), (7, 5), (64, 100), (33, 64), (2, 2)]      # (A, D), batch of 3
SPECTRA_CASES = [(c, a, d) for c in (1, 3) for (a, d) in ((30, 34), (64, 100), (6, 200), (120, 120))]    # n_pairs = 4
RINGPP_SHAPE = (6, 60, 34)
TRANSLATION_SHAPES = [(1, 120, 120), (2, 30, 34), (1, 17, 130), (6, 40, 64)]            # (C, H, W)
DISCO_CASES = [(1, 40, 120, 16), (3, 32, 32, 16), (2, 33, 47, 8), (1, 41, 120, 16), (5, 16, 20, 4)]      # (H, R, S, col)
RELORI_SHAPES = [(33, 47), (16, 20)]
BEV_TRANSLATION_SHAPES = [(6, 120, 120), (1, 48, 80), (2, 33, 47), (3, 16, 20)]         # (C, H, W)
ROTATE_SHAPES = [(2, 48, 80), (1, 33, 47)]
ROTATE_ANGLES = (0.3, -1.1, 2.0)       # radians, one per image of a call


# -------------------------------------------------------------------------------------------------------------------------------- inputs
def normalize(x):
    """(x - mean) / std with the unbiased std over the whole array, float64"""
    x = np.asarray(x, np.float64)
    return (x - x.mean()) / x.std(ddof=1)


def sparse(rng, shape, density=0.3):
    return rng.uniform(size=shape) * (rng.uniform(size=shape) < density)


def entry(seed, i, shape):
    """database entry i of a family: a sparse random image at density 0.3, jointly normalised, float32 [C,A,D]"""
    return normalize(sparse(np.random.default_rng([seed, i]), shape)).astype(np.float32)


def rolled(x, k, rng, axis=1, noise=0.01):
    return (np.roll(x, k, axis=axis) + noise * rng.normal(size=x.shape)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def sweep_case(shape):
    """(query [3,C,A,D], db [6,C,A,D], planted [(q, entry, roll)]) for one of SWEEP_SHAPES"""
    C, A, D = shape
    rng = np.random.default_rng(100 + A + D + C)
    db = np.stack([entry(7, i, shape) for i in range(6)])
    q = np.stack([rolled(db[1], 7, rng), rolled(db[4], -11, rng), rolled(db[5], A // 2, rng)])
    db[2] = rolled(q[0], 0, rng)                           # roll 0: a noisy copy of query 0 itself
    return _ro(q), _ro(db), [(0, 1, 7), (0, 2, 0), (1, 4, -11), (2, 5, A // 2)]


@functools.lru_cache(maxsize=None)
def many_case(name, num_cu):
    """(query [Q,C,A,D], db [N,C,A,D], planted) for one of MANY: queries are rolled, noisy copies of chosen entries"""
    C, A, D, Q, nfn = MANY[name]
    N = nfn(num_cu)
    shape = (C, A, D)
    rng = np.random.default_rng(200 + Q + C + A)
    db = np.stack([entry(11, i, shape) for i in range(N)])
    picks = [N - 3, 0, N // 2, 17, N - 1][:Q]
    rolls = [7, -11, A // 2, 0, 7][:Q]
    q = np.stack([rolled(db[e], k, rng) for e, k in zip(picks, rolls)])
    return _ro(q), _ro(db), [(i, e, k) for i, (e, k) in enumerate(zip(picks, rolls))]


@functools.lru_cache(maxsize=None)
def tie_case(shape):
    """(x, y): x has period A/2 along the angle axis, y is a rolled noisy copy: s[n] and s[n + A/2] are the same sums"""
    C, A, D = shape
    rng = np.random.default_rng(300 + A)
    half = sparse(rng, (C, A // 2, D))
    x = normalize(np.concatenate([half, half], 1)).astype(np.float32)
    assert np.array_equal(x[:, :A // 2], x[:, A // 2:])
    return _ro(x[None]), _ro(rolled(x, -4, rng)[None])


@functools.lru_cache(maxsize=None)
def dft_case(shape):
    A, D = shape
    return _ro(normalize(sparse(np.random.default_rng(400 + A + D), (3, A, D)) + 0.05).astype(np.float32))


@functools.lru_cache(maxsize=None)
def spectra_case(case):
    """(a, b) complex64 [4,C,A,D], non-Hermitian; pair p of b is a (the angle-axis DFT of a complex field) rolled by a planted shift"""
    C, A, D = case
    rng = np.random.default_rng(500 + C + A + D)
    f = rng.normal(size=(4, C, A, D)) * (rng.uniform(size=(4, C, A, D)) < 0.3) + 1j * 0.5 * rng.normal(size=(4, C, A, D))
    g = np.stack([np.roll(f[p], k, axis=1) for p, k in enumerate(spectra_rolls(A))]) + 0.01 * rng.normal(size=f.shape)
    a = np.fft.fft(g, axis=2) / np.sqrt(A)
    b = np.fft.fft(f, axis=2) / np.sqrt(A)
    return _ro(a.astype(np.complex64)), _ro(b.astype(np.complex64))


def spectra_rolls(A):
    return [0, 2, -1, A // 2]


@functools.lru_cache(maxsize=None)
def ringpp_case():
    rng = np.random.default_rng(600)
    a = sparse(rng, RINGPP_SHAPE).astype(np.float32)
    b = (np.roll(a, 13, axis=1) + 0.01 * np.abs(rng.normal(size=a.shape))).astype(np.float32)
    return _ro(a), _ro(b)


def row_plant(H, W):
    """the planted per-row shift: the sinogram of an image moved by (4.6, -2.7) moves row i by about x cos(th_i) + y sin(th_i)"""
    th = np.linspace(0, 2 * np.pi, H)
    return np.rint(4.6 * np.cos(th) - 2.7 * np.sin(th)).astype(int)


@functools.lru_cache(maxsize=None)
def translation_case(shape):
    C, H, W = shape
    rng = np.random.default_rng(700 + H + W)
    q = sparse(rng, shape).astype(np.float32)
    sh = row_plant(H, W)
    p = np.stack([np.roll(q[:, i], sh[i], axis=-1) for i in range(H)], 1) + 0.01 * rng.normal(size=shape)
    return _ro(q), _ro(p.astype(np.float32)), sh


def disco_rolls(R, S):
    """(ring roll, sector roll) per BEV of a DiSCO case; entry 0 is the base"""
    return [(0, 0), (0, 7), (3, -5), (-2, S // 2), (R // 2, 1)]


@functools.lru_cache(maxsize=None)
def disco_case(case):
    """BEVs float32 [5,H,R,S]: a sparse occupancy grid and copies rolled along ring and sector axes"""
    H, R, S, col = case
    rng = np.random.default_rng(800 + R + S)
    base = (rng.uniform(size=(H, R, S)) > 0.85).astype(np.float32)
    return _ro(np.stack([np.roll(np.roll(base, dr, axis=1), ds, axis=2) for dr, ds in disco_rolls(R, S)]))


@functools.lru_cache(maxsize=None)
def spectra_of_disco(case):
    """the float64 reference spectra of disco_case, narrowed to complex64 [5,1,R,S]: the shared INPUT of the phase_corr / calc_rel_ori tests"""
    return _ro(disco_ref(disco_case(case), case[3])[1].astype(np.complex64))


@functools.lru_cache(maxsize=None)
def relori_case(shape):
    """spectra complex64 [3,R,S] of a sparse real-valued grid and two rolled, noisy copies.  The literal cross term is no conjugate
    product: its map is (corr(m) + corr(-m)) / 2 + (conv(m) - conv(-m)) / 2, so a roll by k peaks at +k AND -k and only the convolution part
    decides between them -- on a binary grid that is a tie to rounding; real values and noise give the clear peak the margin test asks for."""
    R, S = shape
    rng = np.random.default_rng(900 + R + S)
    base = sparse(rng, (1, R, S), 0.15)
    bevs = np.stack([np.roll(base, k, axis=2) + (0.02 * rng.uniform(size=base.shape) if k else 0) for k in (0, 3, -6)]).astype(np.float32)
    return _ro(disco_ref(bevs, 2)[1][:, 0].astype(np.complex64))


def bev_plants():
    return [(9, -14), (0, 3), (0, 0), (-5, 6)]           # (dy, dx): rolls along H and W


@functools.lru_cache(maxsize=None)
def bev_translation_case(shape):
    C, H, W = shape
    rng = np.random.default_rng(1000 + H + W)
    a = np.abs(rng.normal(size=shape))
    a[a < 1.2] = 0
    b = np.stack([np.roll(np.roll(a, dy, axis=1), dx, axis=2) + 0.01 * rng.normal(size=shape) for dy, dx in bev_plants()])
    return _ro(np.stack([a] * len(bev_plants())).astype(np.float32)), _ro(b.astype(np.float32))


def _ro(x):
    x.setflags(write=False)
    return x


# ---------------------------------------------------------------------------------------------------------------- RING correlation (sweep)
def ring_corr_ref(q, db, pairwise=False):
    """The sinogram-domain correlation of ring.hip's header: s[n] = A^-1/2 sum_c sum_d | sum_j x[c,(j+n)%A,d] y[c,j,d] |, fftshift-ed.
    q [Q,C,A,D], db [N,C,A,D] -> (corr [Q,N,A] float64 in shifted order, allow [Q,N,A]); pairwise: q[i] against db[i] only -> [Q,1,A]."""
    q, db = np.asarray(q, np.float64), np.asarray(db, np.float64)
    Q, C, A, D = q.shape
    fd, fda = np.fft.rfft(db, axis=2), np.fft.rfft(np.abs(db), axis=2)
    corr, allow = [], []
    for i in range(Q):
        sel = slice(i, i + 1) if pairwise else slice(None)
        c = np.fft.irfft(np.fft.rfft(q[i], axis=1)[None] * np.conj(fd[sel]), n=A, axis=2)            # [N,C,A,D]: sum_j x[(j+n)] y[j]
        ca = np.fft.irfft(np.fft.rfft(np.abs(q[i]), axis=1)[None] * np.conj(fda[sel]), n=A, axis=2)
        corr.append(np.abs(c).sum((1, 3)) / np.sqrt(A))
        allow.append(2 * (A + C + 12) * U * np.abs(ca).sum((1, 3)) / np.sqrt(A))
    return np.fft.fftshift(np.stack(corr), axes=-1), np.fft.fftshift(np.stack(allow), axes=-1)


def peak(corr, denom, allow=None):
    """first argmax m over the last axis, angle = A/2 - m, dist = 1 - max / denom (and allow_dist when allow is given)"""
    A = corr.shape[-1]
    m = np.argmax(corr, -1)
    mx = np.max(corr, -1)
    out = (A // 2 - m, 1.0 - mx / denom)
    if allow is not None:
        out += (np.max(allow, -1) / denom + 4 * U * np.maximum(1.0, mx / denom),)
    return out


def margin(v, allow):
    """(top - second of v, the largest allowance): the planted-case condition is top - second > 10 * allowance"""
    s = np.sort(np.ravel(v))
    return s[-1] - s[-2], float(np.max(allow))


# ------------------------------------------------------------------------------------------------------------------------------ small DFTs
def _trig(N):
    ang = 2 * np.pi * np.outer(np.arange(N), np.arange(N)) / N
    return np.abs(np.cos(ang)) + np.abs(np.sin(ang))


def dft_angle_ref(x):
    """ortho DFT along the angle axis of real [..., A, D]: (complex128 [..., A, D], allow on the complex error)"""
    x = np.asarray(x, np.float64)
    A = x.shape[-2]
    return np.fft.fft(x, axis=-2) / np.sqrt(A), 2 * (A + 8) * U / np.sqrt(A) * np.einsum("kj,...jd->...kd", _trig(A), np.abs(x))


def dft_row_mag_ref(x):
    """|ortho DFT along the detector axis| of real [..., A, D]: (float64, allow)"""
    x = np.asarray(x, np.float64)
    D = x.shape[-1]
    return np.abs(np.fft.fft(x, axis=-1)) / np.sqrt(D), 2 * (D + 8) * U / np.sqrt(D) * np.einsum("kj,...aj->...ak", _trig(D), np.abs(x))


def corr_spectra_ref(a, b):
    """Literal fast_corr on complex spectra a, b [P,C,A,D]: |ortho inverse DFT over the angle axis of a conj(b)|, summed over C and D,
    fftshift-ed: (corr [P,A], allow [P,A]).  dist uses denom = 0.15 A D (no channel factor)."""
    a, b = np.asarray(a, np.complex128), np.asarray(b, np.complex128)
    P, C, A, D = a.shape
    corr = np.abs(np.fft.ifft(a * np.conj(b), axis=2) * np.sqrt(A)).sum((1, 3))
    zx = np.abs(a.real * b.real) + np.abs(a.imag * b.imag)
    zy = np.abs(a.imag * b.real) + np.abs(a.real * b.imag)
    allow = 2 * (A + C + 24) * U / np.sqrt(A) * np.einsum("nk,pckd->pn", _trig(A), zx + zy)
    return np.fft.fftshift(corr, axes=-1), np.fft.fftshift(allow, axes=-1)


def ringpp_ref(a, b):
    """fast_corr_RINGplusplus: joint normalisation of each argument, then the sweep correlation with denom = 0.15 C A D"""
    corr, allow = ring_corr_ref(normalize(a)[None], normalize(b)[None])
    return corr[0, 0], allow[0, 0]


# ----------------------------------------------------------------------------------------------------------------------- solve_translation
def row_corr_ref(q, p):
    """per row i: sum_c | W^-1/2 sum_j q[c,i,(j+n)%W] p[c,i,j] |, fftshift-ed over the lag: (corr [H,W], allow [H,W])"""
    q, p = np.asarray(q, np.float64), np.asarray(p, np.float64)
    C, H, W = q.shape
    c = np.fft.irfft(np.fft.rfft(q, axis=-1) * np.conj(np.fft.rfft(p, axis=-1)), n=W, axis=-1)
    ca = np.fft.irfft(np.fft.rfft(np.abs(q), axis=-1) * np.conj(np.fft.rfft(np.abs(p), axis=-1)), n=W, axis=-1)
    return (np.fft.fftshift(np.abs(c).sum(0), axes=-1) / np.sqrt(W),
            np.fft.fftshift(2 * (W + C + 4) * U / np.sqrt(W) * np.abs(ca).sum(0), axes=-1))


def row_shifts_ref(q, p):
    corr, _ = row_corr_ref(q, p)
    return q.shape[-1] // 2 - np.argmax(corr, -1)


def lstsq_ref(shifts, rot_angle):
    """the 2-unknown least squares [cos(th_i + psi) sin(th_i + psi)] [x y]^T = b_i by the float64 pseudo-inverse: (x, y, residual norm)"""
    H = len(shifts)
    ang = np.linspace(0, 2 * np.pi, H).astype(np.float32).astype(np.float64) + rot_angle
    Amat = np.stack([np.cos(ang), np.sin(ang)], 1)
    sol = np.linalg.pinv(Amat) @ np.asarray(shifts, np.float64)
    return sol[0], sol[1], np.linalg.norm(Amat @ sol - shifts)


# ------------------------------------------------------------------------------------------------------------------ rocFFT-backed operations
def bev_translation_ref(a, b, num_ring, num_sector):
    """solve_translation_bev: joint normalisation, |ifft2(fft2(a) conj(fft2(b)))| (ortho), summed over channels, fftshift, FIRST global
    maximum in row-major order: (y, x, -max, map [H,W])"""
    a, b = normalize(a), normalize(b)
    n = np.sqrt(a.shape[-2] * a.shape[-1])
    c = np.fft.ifft2((np.fft.fft2(a) / n) * np.conj(np.fft.fft2(b) / n)) * n
    m = np.fft.fftshift(np.abs(c).sum(0))
    ix, iy = np.unravel_index(int(np.argmax(m)), m.shape)
    return num_ring // 2 - int(iy), int(ix) - num_sector // 2, -float(m.max()), m


def shift_ceil(x):
    """DiSCO's fftshift2d: shifted[r][s] = x[(r + ceil(R/2)) % R][(s + ceil(S/2)) % S] over the last two axes"""
    R, S = x.shape[-2:]
    return np.roll(x, (-((R + 1) // 2), -((S + 1) // 2)), axis=(-2, -1))


def disco_ref(bev, col):
    """bev [B,H,R,S] -> (signature [B,4 col^2], spectrum complex128 [B,1,R,S]): height sum, ortho fft2, sqrt(|.|^2 + 1e-15), shift, centre crop"""
    x = np.asarray(bev, np.float64).sum(1)
    B, R, S = x.shape
    spec = np.fft.fft2(x) / np.sqrt(R * S)
    mag = shift_ceil(np.sqrt(spec.real ** 2 + spec.imag ** 2 + 1e-15))
    return mag[:, R // 2 - col:R // 2 + col, S // 2 - col:S // 2 + col].reshape(B, -1), spec[:, None]


def phase_corr_ref(a, b):
    """a, b complex [P,1,R,S] -> (map [P,R,S], flat argmax [P]): sqrt(|ifft2(a conj(b), ortho)|^2 + 1e-15), DiSCO shift"""
    a, b = np.asarray(a, np.complex128)[:, 0], np.asarray(b, np.complex128)[:, 0]
    c = np.fft.ifft2(a * np.conj(b)) * np.sqrt(a.shape[-2] * a.shape[-1])
    m = shift_ceil(np.sqrt(c.real ** 2 + c.imag ** 2 + 1e-15))
    return m, m.reshape(m.shape[0], -1).argmax(1)


def relori_ref(a, b):
    """The literal calcRelOri on complex64 a, b [P,R,S]: cross = (ra rb + ia ib) + i (ra ib + rb ia) from FLOAT products (the + in the
    imaginary part is the reference's), unnormalised backward 2-D transform in double, real part: (map float64 [P,R,S], allow [P]).
    The kernel narrows the real part to float and may contract a product into an fma: allow = 2 u (sum of |products| + max |map|)."""
    a, b = np.asarray(a, np.complex64), np.asarray(b, np.complex64)
    ra, ia, rb, ib = a.real, a.imag, b.real, b.imag
    cross = (ra * rb + ia * ib).astype(np.float64) + 1j * (ra * ib + rb * ia).astype(np.float64)
    real = (np.fft.ifft2(cross) * (a.shape[-2] * a.shape[-1])).real
    prods = (np.abs(ra * rb) + np.abs(ia * ib) + np.abs(ra * ib) + np.abs(rb * ia)).astype(np.float64).sum((-2, -1))
    return real, 2 * U * (prods + np.abs(real).max((-2, -1)))


def relori_angle(real):
    """relAngle = (first argmax of the float-narrowed map % width) * 3.0"""
    S = real.shape[-1]
    return np.array([float(int(np.argmax(r.astype(np.float32))) % S) * 3.0 for r in real], np.float32)


def rel_l2(got, ref):
    """||got - ref||_2 / ||ref||_2 over the whole array: the measure in which the rocFFT-backed values are held to 4 x the fp32 CPU restatement.
    The largest single error will not do for that comparison: the spectrum of a non-negative image has one bin (DC) tens of times larger than
    the rest, and the rounding of that one stored value (0 to 2 u of it: the scale constant and the product) exceeds the transform's own error
    in every other bin, so the largest error compares the luck of two roundings, not two transforms.  The L2 norm is the usual accuracy figure
    of an FFT; a wrong, dropped or misplaced element still shows in it at full size (one bin of typical size among N raises it by N^-1/2,
    against errors of 1e-7).  The element-by-element check stays, at the earlier tests' tolerance (FFT_FORMS)."""
    got, ref = np.asarray(got), np.asarray(ref)
    return float(np.linalg.norm((got - ref).ravel()) / np.linalg.norm(ref.ravel()))


# element-by-element tolerances of the earlier DiSCO / BEV tests, |got - ref| <= atol_factor * max |ref| + rtol * |ref|: (rtol, atol_factor)
FFT_FORMS = {"phase_corr": (1e-4, 1e-4), "bev_translation": (2e-4, 2e-4)}


def fft_allow(ref, form):
    """the largest element-wise allowance of a rocFFT-backed map (what the peak margins of its planted cases are held against)"""
    rtol, af = FFT_FORMS[form]
    return (af + rtol) * float(np.abs(ref).max())


# --------------------------------------------------------------------------------------------------------------------------------- rotation
def texel_distance(H, W, ang, yy, xx):
    """float64 distance of output pixel (yy, xx)'s source coordinate from the nearest texel boundary, for the inverse map of either handedness"""
    px, py = xx + 0.5 - 0.5 * W, yy + 0.5 - 0.5 * H
    near = []
    for rot in (ang, -ang):
        sx = np.cos(rot) * px + np.sin(rot) * py + 0.5 * W
        sy = -np.sin(rot) * px + np.cos(rot) * py + 0.5 * H
        near.append(min(abs(sx - np.rint(sx)), abs(sy - np.rint(sy))))
    return min(near)


def rotate_ref(img, ang):
    """torchvision rotate(img, angle) defaults (nearest, about the centre, zero fill) in float64: output pixel centres are turned by
    -angle about the image centre and the nearest input texel is taken (ties to even, like grid_sample).  img [C,H,W], ang in radians."""
    img = np.asarray(img)
    C, H, W = img.shape
    a, b = np.cos(-ang), np.sin(-ang)
    by, bx = np.meshgrid(np.arange(H) + 0.5 - 0.5 * H, np.arange(W) + 0.5 - 0.5 * W, indexing="ij")
    sx = np.rint(a * bx + b * by + 0.5 * W - 0.5).astype(int)
    sy = np.rint(-b * bx + a * by + 0.5 * H - 0.5).astype(int)
    ok = (sx >= 0) & (sx < W) & (sy >= 0) & (sy < H)
    out = np.zeros_like(img)
    out[:, ok] = img[:, sy[ok], sx[ok]]
    return out
