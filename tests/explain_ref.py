"""Plain numpy restatements of b4r_occlude_rows and b4r_attribution_select (include/b4r.h), for the tests."""
import numpy as np

F32 = np.float32
NEG_INF = F32(-np.inf)


def occlude_rows(tokens_in, len_in, labels, V, mask_id, P, w0, Wc):
    """The occluded rows of the recency indices w0 .. w0 + Wc - 1.  Returns a dict: tokens / mask [U * Wc, L] int64, len [U * Wc] int32,
    positions [U * Wc, P] int64, live / unit_pos / unit_label / removed [U * Wc] int32, unit_item [U * Wc] int64.  labels None: item
    mode."""
    tokens_in = np.asarray(tokens_in, np.int64)
    U, L = tokens_in.shape
    N = U * Wc
    out = dict(tokens=np.zeros((N, L), np.int64), mask=np.zeros((N, L), np.int64), len=np.zeros(N, np.int32),
               positions=np.zeros((N, P), np.int64), live=np.zeros(N, np.int32), unit_pos=np.full(N, -1, np.int32),
               unit_item=np.full(N, -1, np.int64), unit_label=np.full(N, -1, np.int32), removed=np.zeros(N, np.int32))

    def g(tok):
        return int(labels[tok]) if labels is not None and 0 <= tok < V else -1

    for u in range(U):
        ln = int(min(max(int(len_in[u]), 1), L))
        hist = [int(x) for x in tokens_in[u, :ln - 1]]
        lab = [g(t) for t in hist]
        for c in range(Wc):
            n = u * Wc + c
            p = ln - 2 - (w0 + c)
            live, gone = p >= 0, set()
            if live and labels is None:
                gone = {p}
            elif live:
                gp = lab[p]
                live = gp >= 0 and gp not in lab[p + 1:]
                if live:
                    gone = {q for q in range(ln - 1) if lab[q] == gp}
            if not live:
                out["tokens"][n] = tokens_in[u]
                ln_o = ln
            else:
                rest = [hist[q] for q in range(ln - 1) if q not in gone]
                ln_o = len(rest) + 1
                out["tokens"][n, :ln_o] = rest + [mask_id]
                out["live"][n], out["unit_pos"][n], out["unit_item"][n] = 1, p, hist[p]
                out["unit_label"][n] = lab[p]
                out["removed"][n] = len(gone)
            out["mask"][n, :ln_o] = 1
            out["len"][n] = ln_o
            out["positions"][n, 0] = ln_o - 1
    return out


def attribution_select(base_logp, occ_logp, live, m):
    """base_logp [U, K] fp32, occ_logp [U * W, K] fp32, live [U * W] int32 -> (w int32, delta fp32), each [U, K, m]: the live entries by
    (delta descending with -0.0 as +0.0, w ascending); delta is ONE fp32 subtraction."""
    base_logp = np.asarray(base_logp, F32)
    occ_logp = np.asarray(occ_logp, F32)
    live = np.asarray(live)
    U, K = base_logp.shape
    W = occ_logp.shape[0] // max(U, 1)
    out_w = np.full((U, K, m), -1, np.int32)
    out_d = np.full((U, K, m), NEG_INF, F32)
    with np.errstate(over="ignore", invalid="ignore"):
        for u in range(U):
            for i in range(K):
                b = base_logp[u, i]
                entries = []
                for w in range(W):
                    o = occ_logp[u * W + w, i]
                    if live[u * W + w] == 0 or not b > NEG_INF or not o > NEG_INF:
                        continue
                    d = F32(b - o)                                         # both operands are fp32: one rounded fp32 subtraction
                    key = F32(0.0) if d == 0 else d                        # -0.0 counts as +0.0
                    entries.append((-float(key), w, d))
                entries.sort(key=lambda e: e[:2])
                for t, (_, w, d) in enumerate(entries[:m]):
                    out_w[u, i, t], out_d[u, i, t] = w, d
    return out_w, out_d
