"""Test helper (not collected): BN254 and Groth16 written from the mathematics and the snarkjs file formats alone, sharing no code
with boundless_amd/csrc (bn254_arith.hpp, bn254.hip, groth16.cpp).

* Fq, Fr, Fq2 (u^2 = -1) and Fq12 as polynomials over Fq modulo w^12 - 18 w^6 + 82 (so w^6 = 9 + u);
* G1: y^2 = x^3 + 3 over Fq; G2: the twist y^2 = x^3 + 3/(9+u) over Fq2, both in Jacobian coordinates;
* the optimal-ate pairing (a product of Miller loops with one final exponentiation) and a Groth16 verifier in the snarkjs form
  e(-A, B) e(alpha, beta) e(IC0 + sum x_i IC_i, gamma) e(C, delta) = 1;
* a seeded satisfiable R1CS generator, a trusted setup from a seeded trapdoor that writes a `.zkey` (Groth16, the layout of
  boundless_amd/csrc/groth16.cpp's conventions block, restated here from snarkjs), a `.wtns` writer;
* a definitional prover (plain-Python MSMs) and, for larger shapes, the same proof computed through the trapdoor (every key point
  is k*G with k known, so an MSM is one scalar product).
"""
import random
import struct

Q = 21888242871839275222246405745257275088696311157297823662689037894645226208583
R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
MONT = 1 << 256  # Montgomery radix of the zkey encoding


def inv(a, m):
    return pow(a, m - 2, m)


# ---- Fq2 as (c0, c1), u^2 = -1 ----
def f2add(a, b):
    return ((a[0] + b[0]) % Q, (a[1] + b[1]) % Q)


def f2sub(a, b):
    return ((a[0] - b[0]) % Q, (a[1] - b[1]) % Q)


def f2mul(a, b):
    return ((a[0] * b[0] - a[1] * b[1]) % Q, (a[0] * b[1] + a[1] * b[0]) % Q)


def f2neg(a):
    return ((-a[0]) % Q, (-a[1]) % Q)


def f2inv(a):
    d = inv((a[0] * a[0] + a[1] * a[1]) % Q, Q)
    return (a[0] * d % Q, (-a[1]) * d % Q)


def f2pow(a, e):
    r = (1, 0)
    while e:
        if e & 1:
            r = f2mul(r, a)
        a = f2mul(a, a)
        e >>= 1
    return r


XI = (9, 1)
B1 = 3
B2 = f2mul((3, 0), f2inv(XI))


class G1F:
    """field ops of G1's base field (ints mod Q)"""
    zero, one = 0, 1
    add = staticmethod(lambda a, b: (a + b) % Q)
    sub = staticmethod(lambda a, b: (a - b) % Q)
    mul = staticmethod(lambda a, b: a * b % Q)
    inv = staticmethod(lambda a: inv(a, Q))
    b = B1


class G2F:
    zero, one = (0, 0), (1, 0)
    add, sub, mul, inv = staticmethod(f2add), staticmethod(f2sub), staticmethod(f2mul), staticmethod(f2inv)
    b = B2


G1_GEN = (1, 2)
G2_GEN = ((10857046999023057135944570762232829481370756359578518086990519993285655852781,
           11559732032986387107991004021392285783925812861821192530917403151452391805634),
          (8495653923123431417604973247489272438418190587263600148770280649306958101930,
           4082367875863433681332203403145435568316851327593401208105741076214120093531))


def on_curve(F, P):
    if P is None:
        return True
    x, y = P
    return F.mul(y, y) == F.add(F.mul(F.mul(x, x), x), F.b)


# ---- Jacobian (X, Y, Z), affine = (X/Z^2, Y/Z^3); None = infinity in affine ----
def jac(F, P):
    return (F.one, F.one, F.zero) if P is None else (P[0], P[1], F.one)


def jdouble(F, P):
    X, Y, Z = P
    if Z == F.zero or Y == F.zero:
        return (F.one, F.one, F.zero)
    A = F.mul(X, X)
    Bv = F.mul(Y, Y)
    C = F.mul(Bv, Bv)
    t = F.add(X, Bv)
    D = F.sub(F.mul(t, t), F.add(A, C))
    D = F.add(D, D)
    E = F.add(F.add(A, A), A)
    Fv = F.mul(E, E)
    X3 = F.sub(Fv, F.add(D, D))
    C8 = F.add(C, C)
    C8 = F.add(C8, C8)
    C8 = F.add(C8, C8)
    Y3 = F.sub(F.mul(E, F.sub(D, X3)), C8)
    Z3 = F.mul(Y, Z)
    return (X3, Y3, F.add(Z3, Z3))


def jadd(F, P, Qp):
    if P[2] == F.zero:
        return Qp
    if Qp[2] == F.zero:
        return P
    X1, Y1, Z1 = P
    X2, Y2, Z2 = Qp
    Z1Z1 = F.mul(Z1, Z1)
    Z2Z2 = F.mul(Z2, Z2)
    U1 = F.mul(X1, Z2Z2)
    U2 = F.mul(X2, Z1Z1)
    S1 = F.mul(F.mul(Y1, Z2), Z2Z2)
    S2 = F.mul(F.mul(Y2, Z1), Z1Z1)
    if U1 == U2:
        return jdouble(F, P) if S1 == S2 else (F.one, F.one, F.zero)
    H = F.sub(U2, U1)
    Rr = F.sub(S2, S1)
    H2 = F.mul(H, H)
    H3 = F.mul(H2, H)
    U1H2 = F.mul(U1, H2)
    X3 = F.sub(F.sub(F.mul(Rr, Rr), H3), F.add(U1H2, U1H2))
    Y3 = F.sub(F.mul(Rr, F.sub(U1H2, X3)), F.mul(S1, H3))
    Z3 = F.mul(F.mul(Z1, Z2), H)
    return (X3, Y3, Z3)


def affine(F, P):
    if P[2] == F.zero:
        return None
    zi = F.inv(P[2])
    zi2 = F.mul(zi, zi)
    return (F.mul(P[0], zi2), F.mul(P[1], F.mul(zi2, zi)))


def jmul(F, P, k):
    acc = (F.one, F.one, F.zero)
    for bit in bin(k)[2:] if k else "":
        acc = jdouble(F, acc)
        if bit == "1":
            acc = jadd(F, acc, P)
    return acc


def mul(F, P, k):
    return affine(F, jmul(F, jac(F, P), k))


def add(F, P, Qp):
    return affine(F, jadd(F, jac(F, P), jac(F, Qp)))


def neg(F, P):
    return None if P is None else (P[0], F.sub(F.zero, P[1]))


def msm(F, points, scalars):
    """definitional multi-scalar multiplication: sum of k_i * P_i, one double-and-add per term"""
    acc = (F.one, F.one, F.zero)
    for P, k in zip(points, scalars):
        if P is not None and k % R:
            acc = jadd(F, acc, jmul(F, jac(F, P), k % R))
    return affine(F, acc)


class FixedBase:
    """k*G for many k (trusted setup, test tables): 8-bit windows of precomputed multiples j * 2^(8i) * G, one Jacobian addition
    per non-zero window, one batch inversion at the end"""

    def __init__(self, F, G):
        self.F = F
        self.tab = []
        B = jac(F, G)
        for _ in range(32):
            row, P = [(F.one, F.one, F.zero)], (F.one, F.one, F.zero)
            for _ in range(255):
                P = jadd(F, P, B)
                row.append(P)
            self.tab.append(row)
            B = jadd(F, P, B)  # 256 * B

    def many(self, ks):
        F = self.F
        out = []
        for k in ks:
            k %= R
            acc = (F.one, F.one, F.zero)
            i = 0
            while k:
                if k & 255:
                    acc = jadd(F, acc, self.tab[i][k & 255])
                k >>= 8
                i += 1
            out.append(acc)
        # batch inversion of the Z coordinates
        zs = [P[2] for P in out]
        pref, run = [], F.one
        for z in zs:
            pref.append(run)
            if z != F.zero:
                run = F.mul(run, z)
        rinv = F.inv(run)
        res = [None] * len(out)
        for i in range(len(out) - 1, -1, -1):
            if zs[i] == F.zero:
                continue
            zi = F.mul(rinv, pref[i])
            rinv = F.mul(rinv, zs[i])
            zi2 = F.mul(zi, zi)
            res[i] = (F.mul(out[i][0], zi2), F.mul(out[i][1], F.mul(zi2, zi)))
        return res


_FB = {}


def fixed_base(group):
    """the shared FixedBase table of G1 (1) or G2 (2)"""
    if group not in _FB:
        _FB[group] = FixedBase(G1F, G1_GEN) if group == 1 else FixedBase(G2F, G2_GEN)
    return _FB[group]


# ---- Fq12 = Fq[w] / (w^12 - 18 w^6 + 82), lists of 12 ints ----
def f12mul(a, b):
    t = [0] * 23
    for i, x in enumerate(a):
        if x:
            for j, y in enumerate(b):
                t[i + j] += x * y
    for k in range(22, 11, -1):  # w^k = 18 w^(k-6) - 82 w^(k-12)
        c = t[k]
        if c:
            t[k - 6] += 18 * c
            t[k - 12] -= 82 * c
    return [x % Q for x in t[:12]]


F12_ONE = [1] + [0] * 11


def f12pow(a, e):
    r = F12_ONE
    for bit in bin(e)[2:]:
        r = f12mul(r, r)
        if bit == "1":
            r = f12mul(r, a)
    return r


def _emb(e, k):
    """the Fq2 element e = c0 + c1 u (u = w^6 - 9) times w^k, as a sparse {power: coefficient} dict"""
    return {k: (e[0] - 9 * e[1]) % Q, k + 6: e[1] % Q}


def _sparse(*terms):
    out = [0] * 12
    for t in terms:
        for k, v in t.items():
            out[k] = (out[k] + v) % Q
    return out


ATE = 29793968203157093288
FROB_X = f2pow(XI, (Q - 1) // 3)
FROB_Y = f2pow(XI, (Q - 1) // 2)
FROB2_X = f2pow(XI, (Q * Q - 1) // 3)
FROB2_Y = f2pow(XI, (Q * Q - 1) // 2)


def _line(T, S, P):
    """the line through the twisted points T, S (affine Fq2 coordinates; the untwisted point is (x w^2, y w^3)) evaluated at the G1
    point P, as an Fq12 element; tangent when T == S, vertical when they are inverse"""
    (x1, y1), (x2, y2) = T, S
    xp, yp = P
    if x1 != x2:
        m = f2mul(f2sub(y2, y1), f2inv(f2sub(x2, x1)))
    elif y1 == y2:
        m = f2mul(f2mul((3, 0), f2mul(x1, x1)), f2inv(f2add(y1, y1)))
    else:  # x_P - x1 w^2
        return _sparse({0: xp}, {k: (-v) % Q for k, v in _emb(x1, 2).items()})
    # untwisted slope is m w; line = m w (x_P - x1 w^2) - (y_P - y1 w^3) = m x_P w + (y1 - m x1) w^3 - y_P
    return _sparse(_emb(f2mul(m, (xp, 0)), 1), _emb(f2sub(y1, f2mul(m, x1)), 3), {0: (-yp) % Q})


def miller(Qp, P):
    if Qp is None or P is None:
        return F12_ONE
    Rp, f = Qp, F12_ONE
    for i in range(ATE.bit_length() - 2, -1, -1):
        f = f12mul(f12mul(f, f), _line(Rp, Rp, P))
        Rp = add(G2F, Rp, Rp)
        if (ATE >> i) & 1:
            f = f12mul(f, _line(Rp, Qp, P))
            Rp = add(G2F, Rp, Qp)
    (x, y) = Qp
    Q1 = (f2mul((x[0], (-x[1]) % Q), FROB_X), f2mul((y[0], (-y[1]) % Q), FROB_Y))
    nQ2 = (f2mul(x, FROB2_X), f2neg(f2mul(y, FROB2_Y)))
    f = f12mul(f, _line(Rp, Q1, P))
    Rp = add(G2F, Rp, Q1)
    f = f12mul(f, _line(Rp, nQ2, P))
    return f


FINAL_EXP = (Q ** 12 - 1) // R


def pairing_product_is_one(pairs):
    """prod e(P_i, Q_i) == 1 for (G1, G2) pairs: one Miller loop each, one final exponentiation"""
    f = F12_ONE
    for P, Qp in pairs:
        f = f12mul(f, miller(Qp, P))
    return f12pow(f, FINAL_EXP) == F12_ONE


def verify(vk, proof, publics):
    """Groth16 (snarkjs form).  vk: dict alpha1, beta2, gamma2, delta2, ic (list of G1); proof: (A, B, C) affine; publics: ints."""
    A, Bp, C = proof
    if len(publics) + 1 != len(vk["ic"]) or any(not (0 <= x < R) for x in publics):
        return False
    if not (on_curve(G1F, A) and on_curve(G2F, Bp) and on_curve(G1F, C)):
        return False
    vkx = msm(G1F, vk["ic"], [1] + list(publics))
    return pairing_product_is_one([(neg(G1F, A), Bp), (vk["alpha1"], vk["beta2"]), (vkx, vk["gamma2"]), (C, vk["delta2"])])


# ---- roots of unity of Fr ----
def root_of_unity(n):
    """primitive n-th root (n a power of two <= 2^28): 5^((r-1)/n)"""
    return pow(5, (R - 1) // n, R)


def intt(vals):
    n = len(vals)
    w = inv(root_of_unity(n), R)
    ninv = inv(n, R)
    return [sum(v * pow(w, i * k, R) for i, v in enumerate(vals)) * ninv % R for k in range(n)] if n <= 16 else _fft(vals, w, ninv)


def _fft(vals, w, scale=1):
    n = len(vals)
    if n == 1:
        return [vals[0] * scale % R]
    ev = _fft(vals[0::2], w * w % R)
    od = _fft(vals[1::2], w * w % R)
    out = [0] * n
    t = 1
    for k in range(n // 2):
        x = od[k] * t
        out[k] = (ev[k] + x) * scale % R
        out[k + n // 2] = (ev[k] - x) * scale % R
        t = t * w % R
    return out


def coset_eval(coeffs, N):
    """evaluate the polynomial (degree < N) at the odd coset omega_2N^(2j+1), j < N"""
    g = root_of_unity(2 * N)
    shifted = [c * pow(g, k, R) % R for k, c in enumerate(coeffs)]
    return _fft(shifted, root_of_unity(N))


# ---- R1CS / setup / zkey ----
class R1CS:
    """constraints (a, b, c): dicts signal -> coefficient, with <a,w> <b,w> = <c,w>"""

    def __init__(self, n_vars, n_public, constraints):
        self.n_vars, self.n_public, self.constraints = n_vars, n_public, constraints

    def domain(self):
        n = len(self.constraints) + self.n_public + 1
        N = 1
        while N < n:
            N *= 2
        return N

    def satisfied(self, w):
        dot = lambda row: sum(c * w[s] for s, c in row.items()) % R
        return all(dot(a) * dot(b) % R == dot(c) for a, b, c in self.constraints)


def random_r1cs(rng, witness, n_public, n_constraints, width=3):
    """a satisfiable R1CS over the given witness: random sparse A and B rows; the C row makes each constraint hold"""
    n = len(witness)
    cons = []
    nz = [i for i in range(n) if witness[i] % R]
    for _ in range(n_constraints):
        a = {rng.randrange(n): rng.randrange(1, R) for _ in range(rng.randint(1, width))}
        b = {rng.randrange(n): rng.choice([1, R - 1, rng.randrange(1, R)]) for _ in range(rng.randint(1, width))}
        ab = sum(c * witness[s] for s, c in a.items()) * sum(c * witness[s] for s, c in b.items()) % R
        if ab == 0:
            c = {}
        else:
            k = rng.choice(nz)
            c = {k: ab * inv(witness[k], R) % R}
        cons.append((a, b, c))
    return R1CS(n, n_public, cons)


def random_witness(rng, n_vars, kind="random"):
    pool = {"random": lambda: rng.randrange(R), "small": lambda: rng.choice([0, 1, 1, 0, 2, R - 1]),
            "repeat": lambda: rng.choice([7, 7, 7, R - 1, 0, 1]), "edge": lambda: rng.choice([0, 1, R - 1, 7])}[kind]
    return [1] + [pool() for _ in range(n_vars - 1)]


def lagrange_at(tau, N, shift=1):
    """L_j(tau) over the domain {shift * omega_N^j}, j < N"""
    w = root_of_unity(N)
    zt = (pow(tau, N, R) - pow(shift, N, R)) % R
    out, pt = [], shift % R
    for _ in range(N):
        # L_j(x) = (x^N - s^N) / (N * pt^(N-1) * (x - pt)),  pt^(N-1) = s^N / pt
        den = N * pow(shift, N, R) * inv(pt, R) % R * (tau - pt) % R
        out.append(zt * inv(den, R) % R)
        pt = pt * w % R
    return out


class Setup:
    """A Groth16 trusted setup from a seeded trapdoor; `scalars` keeps every key point's discrete log."""

    def __init__(self, r1cs, seed):
        rng = random.Random(seed)
        self.r1cs = r1cs
        self.tau, self.alpha, self.beta, self.gamma, self.delta = (rng.randrange(2, R) for _ in range(5))
        N = r1cs.domain()
        self.N = N
        n, npub = r1cs.n_vars, r1cs.n_public
        L = lagrange_at(self.tau, N)
        u, v, wv = [0] * n, [0] * n, [0] * n
        coefs = []
        for ci, (a, b, c) in enumerate(r1cs.constraints):
            for s, k in a.items():
                u[s] = (u[s] + k * L[ci]) % R
                coefs.append((0, ci, s, k))
            for s, k in b.items():
                v[s] = (v[s] + k * L[ci]) % R
                coefs.append((1, ci, s, k))
            for s, k in c.items():
                wv[s] = (wv[s] + k * L[ci]) % R
        m = len(r1cs.constraints)
        for s in range(npub + 1):  # snarkjs: one extra A-row per public signal (and the constant one)
            u[s] = (u[s] + L[m + s]) % R
            coefs.append((0, m + s, s, 1))
        self.coefs = coefs
        self.u, self.v = u, v
        gi, di = inv(self.gamma, R), inv(self.delta, R)
        lin = [(self.beta * u[i] + self.alpha * v[i] + wv[i]) % R for i in range(n)]
        self.ic_k = [lin[i] * gi % R for i in range(npub + 1)]
        self.c_k = [lin[i] * di % R for i in range(npub + 1, n)]
        Lc = lagrange_at(self.tau, N, shift=root_of_unity(2 * N))
        zt = (pow(self.tau, N, R) - 1) % R
        f = zt * inv((-2 * self.delta) % R, R) % R
        self.h_k = [lj * f % R for lj in Lc]
        g1, g2 = fixed_base(1), fixed_base(2)
        self.alpha1, self.beta1, self.delta1 = g1.many([self.alpha, self.beta, self.delta])
        self.beta2, self.gamma2, self.delta2 = g2.many([self.beta, self.gamma, self.delta])
        self.A, self.B1, self.C, self.H, self.IC = (g1.many(ks) for ks in (u, v, self.c_k, self.h_k, self.ic_k))
        self.B2 = g2.many(v)

    def vk(self):
        return {"alpha1": self.alpha1, "beta2": self.beta2, "gamma2": self.gamma2, "delta2": self.delta2, "ic": self.IC}

    def zkey(self):
        return write_zkey(self)


def _fq_le(x):
    return (x * MONT % Q).to_bytes(32, "little")


def g1_bytes(P):
    return bytes(64) if P is None else _fq_le(P[0]) + _fq_le(P[1])


def g2_bytes(P):
    return bytes(128) if P is None else b"".join(_fq_le(c) for c in (P[0][0], P[0][1], P[1][0], P[1][1]))


def _section(t, data):
    return struct.pack("<IQ", t, len(data)) + data


def write_zkey(s):
    r1 = s.r1cs
    hdr = (struct.pack("<I", 32) + Q.to_bytes(32, "little") + struct.pack("<I", 32) + R.to_bytes(32, "little")
           + struct.pack("<III", r1.n_vars, r1.n_public, s.N)
           + g1_bytes(s.alpha1) + g1_bytes(s.beta1) + g2_bytes(s.beta2) + g2_bytes(s.gamma2) + g1_bytes(s.delta1) + g2_bytes(s.delta2))
    r2 = MONT * MONT % R
    coefs = struct.pack("<I", len(s.coefs)) + b"".join(struct.pack("<III", m, c, sig) + (k * r2 % R).to_bytes(32, "little")
                                                       for m, c, sig, k in s.coefs)
    secs = [(1, struct.pack("<I", 1)), (2, hdr), (3, b"".join(map(g1_bytes, s.IC))), (4, coefs), (5, b"".join(map(g1_bytes, s.A))),
            (6, b"".join(map(g1_bytes, s.B1))), (7, b"".join(map(g2_bytes, s.B2))), (8, b"".join(map(g1_bytes, s.C))),
            (9, b"".join(map(g1_bytes, s.H))), (10, b"")]
    return b"zkey" + struct.pack("<II", 1, len(secs)) + b"".join(_section(t, d) for t, d in secs)


def write_wtns(witness):
    hdr = struct.pack("<I", 32) + R.to_bytes(32, "little") + struct.pack("<I", len(witness))
    vals = b"".join((x % R).to_bytes(32, "little") for x in witness)
    return b"wtns" + struct.pack("<II", 2, 2) + _section(1, hdr) + _section(2, vals)


def witness_bytes(witness):
    return b"".join((x % R).to_bytes(32, "little") for x in witness)


# ---- provers ----
def h_values(s, witness):
    """p_j = (A B - C)(omega_2N^(2j+1)) from the coefficient list, as the zkey's H section expects"""
    N = s.N
    a, b = [0] * N, [0] * N
    for m, c, sig, k in s.coefs:
        (a if m == 0 else b)[c] = ((a if m == 0 else b)[c] + k * witness[sig]) % R
    cc = [x * y % R for x, y in zip(a, b)]
    ea, eb, ec = (coset_eval(intt(vals), N) for vals in (a, b, cc))
    return [(x * y - z) % R for x, y, z in zip(ea, eb, ec)]


def prove(s, witness, r, sk, definitional=True):
    """The Groth16 proof for fixed r, s.  definitional=True: plain MSMs over the key's points (small keys); False: the same sums
    through the trapdoor's discrete logs (one scalar product per point, any size)."""
    n, npub = s.r1cs.n_vars, s.r1cs.n_public
    p = h_values(s, witness)
    wc = witness[npub + 1:]
    if definitional:
        A = msm(G1F, s.A + [s.alpha1, s.delta1], witness + [1, r])
        B2 = msm(G2F, s.B2 + [s.beta2, s.delta2], witness + [1, sk])
        B1 = msm(G1F, s.B1 + [s.beta1, s.delta1], witness + [1, sk])
        C = msm(G1F, s.C + s.H + [A, B1, s.delta1], wc + p + [sk, r, (-r * sk) % R])
        return A, B2, C
    dot = lambda ks, ws: sum(k * w for k, w in zip(ks, ws)) % R
    a = (s.alpha + dot(s.u, witness) + r * s.delta) % R
    b = (s.beta + dot(s.v, witness) + sk * s.delta) % R
    c = (dot(s.c_k, wc) + dot(s.h_k, p) + sk * a + r * b - r * sk * s.delta) % R
    return mul(G1F, G1_GEN, a), mul(G2F, G2_GEN, b), mul(G1F, G1_GEN, c)
