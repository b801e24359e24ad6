"""The plain reference of GBLUP prediction ("GBLUP prediction"): numpy.longdouble throughout, from the stored draws
U, the set's K and the raw genotypes of the records (Z) and of the candidates (Zc).  Nothing here knows the device's orders."""
import numpy as np

EPS = 2.0 ** -53
L = np.longdouble


def reference(Z, Zc, K, U, method):
    """C, m (Nc x T), sum, sumsq, s, gcc, beta-sum of the back-solve, and the absolute sums the bounds are made of: A_ci =
    sum_j d_j |z_cj - mu_j| |z_ij - mu_j|, B_it = sum_k |K_ik| |u_kt|, and Bs = sum_j |z_cj - mu_j| d_j sum_i |z_ij - mu_j| B_it summed over t."""
    Z, Zc, K, U = (np.asarray(a).astype(L) for a in (Z, Zc, K, U))
    N, P = Z.shape
    mu = Z.sum(axis=0) / N
    tp = mu * (1 - mu / 2)
    d = np.full(P, 1 / tp.sum()) if method == 1 else 1 / (P * tp)
    X, Xc = Z - mu, Zc - mu
    C = (Xc * d) @ X.T
    gcc = (d * Xc * Xc).sum(axis=1)
    W = K @ U
    m = C @ W
    s = gcc - ((C @ K) * C).sum(axis=1)
    A, B = (np.abs(Xc) * d) @ np.abs(X).T, np.abs(K) @ np.abs(U)
    beta_sum = (d[:, None] * (X.T @ W)).sum(axis=1)
    return dict(C=C, m=m, sum=m.sum(axis=1), sumsq=(m * m).sum(axis=1), s=s, gcc=gcc, A=A, B=B, AKA=((A @ np.abs(K)) * A).sum(axis=1),
                Xc=Xc, beta_sum=beta_sum, beta_abs=np.abs(Xc) @ (d[:, None] * (np.abs(X).T @ B)).sum(axis=1))
