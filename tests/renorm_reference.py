"""Float64 numpy reference of the renorm ('dr') site's small-matrix stage, shared by tests/test_renorm_cpu.py and
tests/test_renorm_gpu.py (not collected: no test_ prefix).  DESIGN.md section 4.15; row-vector convention of SURVEY row a10."""
import numpy as np


def phi(X):
    """Lower triangle with the diagonal halved."""
    P = np.tril(X)
    P[np.diag_indices_from(P)] *= 0.5
    return P


def factor_backward(R, gsum, W, Wm, C0, gamma, A, M, eps, ddof=1):
    """What wc_bwd_factor_renorm_f64 computes -> (dgamma, dbeta, S, gmean):
        dgamma_k = W_m R_k;  Wbar_eff = sum_k Gamma_k R_k^T;  P = -Phi(C0^T Wbar_eff W^T);  S = 2 (1 - eps) / (M - ddof) sym(W^T P W);
        gmean = (1 / M) sum_k gsum_k A_k^T."""
    dgamma = np.einsum('ij,kjo->kio', Wm, R)
    Wbar_eff = np.einsum('kij,klj->il', gamma, R)
    P = -phi(C0.T @ Wbar_eff @ W.T)
    Q = W.T @ P @ W
    S = 2.0 * (1.0 - eps) / (M - ddof) * 0.5 * (Q + Q.T)
    gmean = np.einsum('kj,kcj->c', gsum, A) / M
    return dgamma, np.array(gsum, np.float64), S, gmean
