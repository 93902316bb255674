"""Regenerates the constant tables of rotationnormflow_amd/csrc/fisher_exact.h with mpmath (40 digits) and prints them as C initialisers:

  * the 16-point Gauss-Legendre rule on [0, 1]: H[i] = (1 + x_i) / 2 and W[i] = w_i / 2;
  * the Taylor coefficients 1 / (k!)^2 and 1 / (k! (k+1)!) of I0 and I1 in t = x^2 / 4 (x <= 8);
  * Chebyshev coefficients in w = 16 / x - 1 of sqrt(x) exp(-x) I0(x) and sqrt(x) exp(-x) I1(x) for x >= 8, cut where they fall under
    1e-18 (c_0 is stored halved, ready for Clenshaw's recurrence).

Usage: python tools/gen_fisher_exact_tables.py
"""
import mpmath as mp
from numpy.polynomial.legendre import leggauss

mp.mp.dps = 40
N_SMALL = 25            # terms of the Taylor series: 16^24 / (24!)^2 = 2e-19 against I0(8) = 427
N_FIT = 48              # Chebyshev nodes of the fit for x >= 8


def gauss_legendre(n):
    xs, ws = [], []
    for start in leggauss(n)[0]:
        x = mp.findroot(lambda t: mp.legendre(n, t), mp.mpf(float(start)))
        d = n * (x * mp.legendre(n, x) - mp.legendre(n - 1, x)) / (x * x - 1)
        xs.append(x)
        ws.append(2 / ((1 - x * x) * d * d))
    return xs, ws


def cheb_coeffs(f, n):
    nodes = [mp.cos(mp.pi * (j + mp.mpf(1) / 2) / n) for j in range(n)]
    vals = [f(w) for w in nodes]
    return [2 * mp.fsum(vals[j] * mp.cos(mp.pi * k * (j + mp.mpf(1) / 2) / n) for j in range(n)) / n for k in range(n)]


def scaled(order):
    def f(w):
        x = 16 / (w + 1)
        return mp.sqrt(x) * mp.exp(-x) * mp.besseli(order, x)
    return f


def show(name, vals):
    print(f"{name}[{len(vals)}] = {{")
    for i in range(0, len(vals), 4):
        print("    " + ", ".join(mp.nstr(v, 17, min_fixed=0, max_fixed=0) for v in vals[i:i + 4]) + ",")
    print("};")


def main():
    x, w = gauss_legendre(16)
    show("GL_H", [(1 + t) / 2 for t in x])
    show("GL_W", [t / 2 for t in w])
    show("I0_SMALL", [1 / mp.factorial(k) ** 2 for k in range(N_SMALL)])
    show("I1_SMALL", [1 / (mp.factorial(k) * mp.factorial(k + 1)) for k in range(N_SMALL)])
    for order in (0, 1):
        c = cheb_coeffs(scaled(order), N_FIT)
        c[0] /= 2
        keep = max(k for k in range(N_FIT) if abs(c[k]) > mp.mpf("1e-18")) + 1
        show(f"I{order}_LARGE", c[:keep])


if __name__ == "__main__":
    main()
