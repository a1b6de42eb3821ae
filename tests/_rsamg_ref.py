"""Plain restatement of the extended+i interpolation loop (the local case: no ghost part), for the tests of
ramd_mat_rs_extpi_interpolation.  Scalar arithmetic in the operator's value type, additions in loop order; the set of a
row is collected first, the weights accumulate in a dict and leave in ascending column order.  tests/test_cpu_rsamg.py
checks this restatement against the goldens recorded from the genuine library."""
import numpy as np


def extpi(rp, ci, va, cf, S, ff1, dtype=np.float64, stats=None):
    """-> (rowptr int32, col int32, val dtype, ncol) of P; stats (a dict) counts the entries a sign test left out"""
    T = np.dtype(dtype).type
    n = len(rp) - 1
    va = np.asarray(va, dtype=dtype)
    zero = T(0)
    diag = np.zeros(n, dtype=dtype)
    for i in range(n):
        for j in range(rp[i], rp[i + 1]):
            if ci[j] == i:
                diag[i] = va[j]
                break
    f2c = np.zeros(n + 1, dtype=np.int64)
    f2c[1:] = np.cumsum(np.asarray(cf[:n]) == 1)
    prp, pci, pval = [0], [], []
    with np.errstate(all="ignore"):
        for i in range(n):
            if cf[i] == 1:
                pci.append(f2c[i]); pval.append(T(1)); prp.append(len(pci))
                continue
            table = {}
            for k in range(rp[i], rp[i + 1]):
                c = ci[k]
                if not S[k] or c == i:
                    continue
                if cf[c] == 1:
                    table[c] = zero
                else:
                    for l in range(rp[c], rp[c + 1]):
                        cc = ci[l]
                        if S[l] and cc != c and cf[cc] == 1:
                            table[cc] = zero
                            if ff1:
                                break
            a_ii = diag[i]
            pos_ii = a_ii >= zero
            sum_k, sum_n = zero, zero
            for k in range(rp[i], rp[i + 1]):
                c = ci[k]
                if c == i:
                    continue
                a_ik = va[k]
                if S[k] and cf[c] == 2:
                    sum_l, a_ki, a_kk = zero, zero, diag[c]
                    for l in range(rp[c], rp[c + 1]):
                        cc, v = ci[l], va[l]
                        pos = v >= zero
                        if cc == i:
                            if pos_ii != pos:
                                sum_l = T(sum_l + v)
                            elif stats is not None:
                                stats["sign_skips"] = stats.get("sign_skips", 0) + 1
                            a_ki = v
                        elif cf[cc] == 1 and cc in table:
                            if pos_ii != pos:
                                sum_l = T(sum_l + v)
                            elif stats is not None:
                                stats["sign_skips"] = stats.get("sign_skips", 0) + 1
                    sum_l = T(a_ik / sum_l)
                    pos_kk = a_kk >= zero
                    for l in range(rp[c], rp[c + 1]):
                        cc, v = ci[l], va[l]
                        if cf[cc] == 1 and pos_kk != (v >= zero) and cc in table:
                            table[cc] = T(table[cc] + T(v * sum_l))
                    if pos_kk != (a_ki >= zero):
                        sum_k = T(sum_k + T(a_ki * sum_l))
                in_c_hat = False
                if cf[c] == 1 and c in table:
                    table[c] = T(table[c] + a_ik)
                    in_c_hat = True
                if not in_c_hat and not S[k]:
                    sum_n = T(sum_n + a_ik)
            a_tilde = T(T(-1) / T(T(sum_n + sum_k) + a_ii))
            for c in sorted(table):
                pci.append(f2c[c]); pval.append(T(a_tilde * table[c]))
            prp.append(len(pci))
    return (np.array(prp, dtype=np.int32), np.array(pci, dtype=np.int32), np.array(pval, dtype=dtype), int(f2c[n]))
