"""numpy reference of the TNS preconditioner and of the Krylov recurrences it is tested in (no GPU, no library).

TNS (truncated Neumann series): with dinv the inverse diagonal as ExtractInverseDiagonal defines it (1 / a_ii, 1 where the
stored a_ii is zero, 0 where no diagonal entry is stored) and K = strict_lower(A) . diag(dinv) (K_ij = a_ij dinv_j),

    M^-1 r = (I - K^T + K^T K^T) diag(dinv) (I - K + K K) r

evaluated in the order of the library's apply:  t1 = K r ; t2 = K t1 ; u = t1 - t2 ; y = (r - u) dinv ;
s1 = K^T y ; s2 = K^T s1 ; x = y - s1 + s2.
"""
import numpy as np

LD = np.longdouble


def inverse_diagonal(rp, ci, va, dtype=LD):
    n = len(rp) - 1
    d = np.zeros(n, dtype=dtype)
    for i in range(n):
        for j in range(rp[i], rp[i + 1]):
            if ci[j] == i:  # the first stored diagonal entry
                d[i] = dtype(1) / dtype(va[j]) if va[j] != 0 else dtype(1)
                break
    return d


def strict_lower_entries(rp, ci):
    """(rows, cols, positions) of the entries with col < row, in storage order"""
    n = len(rp) - 1
    rows = np.repeat(np.arange(n), np.diff(rp))
    pos = np.nonzero(np.asarray(ci) < rows)[0]
    return rows[pos], np.asarray(ci)[pos], pos


def longest_triangle_row(rp, ci):
    """w of the bound: the longest row of K or of K^T"""
    r, c, _ = strict_lower_entries(rp, ci)
    n = len(rp) - 1
    if len(r) == 0:
        return 0
    return int(max(np.bincount(r, minlength=n).max(), np.bincount(c, minlength=n).max()))


def tns_apply(rp, ci, va, r, absolute=False):
    """-> x = M^-1 r in np.longdouble from the CSR arrays as they are (cast nothing: pass float32 arrays for the fp32 case);
    absolute=True: every operand replaced by its absolute value and every subtraction by an addition (the bound's x-bar)"""
    va = np.asarray(va).astype(LD)
    r = np.asarray(r).astype(LD)
    d = inverse_diagonal(rp, ci, va)
    rows, cols, pos = strict_lower_entries(rp, ci)
    k = va[pos] * d[cols]
    sgn = LD(-1)
    if absolute:
        k, r, d, sgn = np.abs(k), np.abs(r), np.abs(d), LD(1)

    def mul(out_idx, in_idx, v):
        out = np.zeros(len(v), dtype=LD)
        np.add.at(out, out_idx, k * v[in_idx])
        return out

    t1 = mul(rows, cols, r)
    t2 = mul(rows, cols, t1)
    u = t1 + sgn * t2
    y = (r + sgn * u) * d
    s1 = mul(cols, rows, y)
    s2 = mul(cols, rows, s1)
    return y + sgn * s1 + s2


def tns_bound(rp, ci, va, r, u):
    """(4 w + 10) u x-bar, element-wise: four dot products of length w and ten element-wise operations"""
    w = longest_triangle_row(rp, ci)
    return (4 * w + 10) * LD(u) * tns_apply(rp, ci, va, r, absolute=True)


def dense_inverse_operator(A):
    """M^-1 as a dense float64 matrix from a dense A with a full non-zero diagonal (the check of tns_apply itself)"""
    n = A.shape[0]
    Dinv = np.diag(1.0 / np.diag(A))
    K = np.tril(A, -1) @ Dinv
    I = np.eye(n)
    return (I - K.T + K.T @ K.T) @ Dinv @ (I - K + K @ K)


def csr_to_dense(rp, ci, va):
    n = len(rp) - 1
    A = np.zeros((n, n))
    for i in range(n):
        for j in range(rp[i], rp[i + 1]):
            A[i, ci[j]] += va[j]
    return A


def csr_matvec(rp, ci, va, x):
    rows = np.repeat(np.arange(len(rp) - 1), np.diff(rp))
    out = np.zeros(len(rp) - 1)
    np.add.at(out, rows, np.asarray(va, dtype=np.float64) * x[np.asarray(ci)])
    return out


def is_bitwise_symmetric(rp, ci, va):
    """rows strictly ascending and A equal to its transpose bit for bit -> (sorted, symmetric)"""
    n = len(rp) - 1
    ent = {}
    for i in range(n):
        cols = ci[rp[i]:rp[i + 1]]
        if np.any(np.diff(cols) <= 0):
            return False, False
        for j in range(rp[i], rp[i + 1]):
            ent[(i, int(ci[j]))] = np.asarray(va[j]).tobytes()
    return True, all(ent.get((j, i)) == b for (i, j), b in ent.items())


# ---------------------------------------------------------------- the Krylov recurrences (fp64), iteration control included
class _Ctrl:
    def __init__(self, abs_tol=1e-15, rel_tol=1e-6, div_tol=1e8, max_iter=1000000):
        self.a, self.r, self.d, self.mx = abs_tol, rel_tol, div_tol, max_iter
        self.it, self.status, self.hist = 0, 0, []

    def init(self, res):
        self.r0 = res
        self.hist.append(res)
        if abs(res) <= self.a:
            self.status = 1
            return False
        return True

    def check(self, res):
        self.it += 1
        self.hist.append(res)
        if abs(res) <= self.a:
            self.status = 1
        elif res / self.r0 <= self.r:
            self.status = 2
        elif self.it >= self.mx:
            self.status = 4
        elif res / self.r0 >= self.d:
            self.status = 3
        return self.status != 0


def cg(A, M, b, max_iter=1000000):
    """preconditioned CG: A, M callables; -> (iterations, status, x, history)"""
    c = _Ctrl(max_iter=max_iter)
    x = np.zeros_like(b)
    r = b - A(x)
    if not c.init(np.linalg.norm(r)):
        return c.it, c.status, x, c.hist
    z = M(r)
    p = z.copy()
    rho = r @ z
    while True:
        q = A(p)
        alpha = rho / (p @ q)
        x = x + alpha * p
        r = r - alpha * q
        if c.check(np.linalg.norm(r)):
            break
        z = M(r)
        rho_old, rho = rho, r @ z
        p = (rho / rho_old) * p + z
    return c.it, c.status, x, c.hist


def bicgstab(A, M, b, max_iter=1000000):
    c = _Ctrl(max_iter=max_iter)
    x = np.zeros_like(b)
    r0 = b - A(x)
    if not c.init(np.linalg.norm(r0)):
        return c.it, c.status, x, c.hist
    r = r0.copy()
    p = r.copy()
    rho = r @ r
    z = M(r)
    while True:
        q = A(z)
        alpha = rho / (r0 @ q)
        r = r - alpha * q
        v = M(r)
        t = A(v)
        omega = (t @ r) / (t @ t)
        if not np.isfinite(omega) or omega == 0.0:
            x = x + alpha * p
            c.check(np.linalg.norm(b - A(x)))
            break
        x = x + alpha * z + omega * v
        r = r - omega * t
        if c.check(np.linalg.norm(r)):
            break
        rho_old, rho = rho, r0 @ r
        if rho == 0.0:
            break
        beta = (rho / rho_old) * (alpha / omega)
        p = beta * p - beta * omega * q + r
        z = M(p)
    return c.it, c.status, x, c.hist


def gmres(A, M, b, basis=30, max_iter=1000000):
    """left-preconditioned restarted GMRES, the residual is that of the preconditioned system"""
    c = _Ctrl(max_iter=max_iter)
    n = len(b)
    x = np.zeros_like(b)
    V = np.zeros((basis + 1, n))
    V[0] = M(b - A(x))
    g = np.zeros(basis + 1)
    g[0] = np.linalg.norm(V[0])
    if not c.init(abs(g[0])):
        return c.it, c.status, x, c.hist
    while True:
        V[0] /= g[0]
        H = np.zeros((basis + 1, basis))
        cs, sn = np.zeros(basis), np.zeros(basis)
        i = 0
        while i < basis:
            w = M(A(V[i]))
            for k in range(i + 1):
                H[k, i] = V[k] @ w
                w = w - H[k, i] * V[k]
            H[i + 1, i] = np.linalg.norm(w)
            V[i + 1] = w / H[i + 1, i]
            for k in range(i):
                H[k, i], H[k + 1, i] = cs[k] * H[k, i] + sn[k] * H[k + 1, i], -sn[k] * H[k, i] + cs[k] * H[k + 1, i]
            den = np.hypot(H[i, i], H[i + 1, i])
            cs[i], sn[i] = H[i, i] / den, H[i + 1, i] / den
            H[i, i], H[i + 1, i] = den, 0.0
            g[i], g[i + 1] = cs[i] * g[i], -sn[i] * g[i]
            i += 1
            if c.check(abs(g[i])):
                break
        y = np.linalg.solve(np.triu(H[:i, :i]), g[:i])
        x = x + y @ V[:i]
        V[0] = M(b - A(x))
        g[:] = 0.0
        g[0] = np.linalg.norm(V[0])
        if c.status != 0:
            break
        if abs(g[0]) <= c.a or g[0] / c.r0 <= c.r:  # CheckResidualNoCount after a full cycle
            c.status = 1 if abs(g[0]) <= c.a else 2
            break
    return c.it, c.status, x, c.hist


# ---------------------------------------------------------------- synthetic symmetric operators for the kernel's edges
def _csr_from_dict(n, ent, dtype=np.float64):
    """ent: {(i, j): value}; rows sorted by column"""
    rp = np.zeros(n + 1, dtype=np.int32)
    keys = sorted(ent)
    for i, _ in keys:
        rp[i + 1] += 1
    rp = np.cumsum(rp).astype(np.int32)
    ci = np.array([j for _, j in keys], dtype=np.int32)
    va = np.array([ent[k] for k in keys], dtype=dtype)
    return rp, ci, va


def sym_random(n, per_row=4, seed=0, diag="dominant"):
    """symmetric, random pattern and values; every row has its diagonal"""
    rng = np.random.default_rng(seed)
    ent = {}
    for i in range(n):
        for j in rng.integers(0, n, size=min(per_row, n)):
            if i != j:
                v = float(rng.uniform(-1.0, 1.0))
                ent[(i, int(j))] = v
                ent[(int(j), i)] = v
    for i in range(n):
        s = sum(abs(v) for (r, _), v in ent.items() if r == i)
        ent[(i, i)] = s + float(rng.uniform(0.5, 1.5))
    return _csr_from_dict(n, ent)


def sym_arrow(n=2700, long=2600, seed=1):
    """row 0 has `long` upper entries, row n-1 has `long` lower ones (longer than a staging pass), a tridiagonal in between"""
    rng = np.random.default_rng(seed)
    ent = {}

    def put(i, j):
        v = float(rng.uniform(-1.0, 1.0))
        ent[(i, j)] = v
        ent[(j, i)] = v

    for j in range(1, long + 1):
        put(0, j)
    for j in range(n - 1 - long, n - 1):
        put(n - 1, j)
    for i in range(1, n - 1):
        if (i, i + 1) not in ent:
            put(i, i + 1)
    for i in range(n):
        ent[(i, i)] = float(long) + float(rng.uniform(0.5, 1.5))
    return _csr_from_dict(n, ent)


def sym_empty_triangles(n=200, seed=2):
    """rows with only a diagonal, rows with only upper or only lower entries next to full ones"""
    rng = np.random.default_rng(seed)
    ent = {}
    for i in range(0, n - 3, 7):  # a few 2-row couplings far apart: the lower row has no upper part, the upper row no lower part
        v = float(rng.uniform(-1.0, 1.0))
        ent[(i, i + 3)] = v
        ent[(i + 3, i)] = v
    for i in range(n):
        ent[(i, i)] = float(rng.uniform(1.5, 2.5))
    return _csr_from_dict(n, ent)


def sym_diagonal_holes(n=130, seed=3):
    """some diagonal entries not stored, some stored as zero"""
    rp, ci, va = sym_random(n, per_row=3, seed=seed)
    keep = np.ones(len(ci), dtype=bool)
    rows = np.repeat(np.arange(n), np.diff(rp))
    for i in range(n):
        if i % 5 == 1:
            keep[(rows == i) & (ci == i)] = False
        if i % 7 == 2:
            va[(rows == i) & (ci == i)] = 0.0
    rp2 = np.zeros(n + 1, dtype=np.int32)
    np.cumsum(np.bincount(rows[keep], minlength=n), out=rp2[1:])
    return rp2, ci[keep].copy(), va[keep].copy()


def structurally_symmetric_only(n=65, seed=4, dtype=np.float64):
    """the pattern is symmetric, one value is off by one unit in the last place of `dtype`"""
    rp, ci, va = sym_random(n, per_row=3, seed=seed)
    va = va.astype(dtype)
    rows = np.repeat(np.arange(n), np.diff(rp))
    j = np.nonzero(ci > rows)[0][len(ci) // 5]
    va[j] = np.nextafter(va[j], dtype(np.inf))
    return rp, ci, va
