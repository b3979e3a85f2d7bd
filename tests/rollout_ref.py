"""Plain numpy restatements of b4r_beam_select and b4r_rollout_advance (include/b4r.h), for the tests."""
import numpy as np

F32 = np.float32
NEG_INF = F32(-np.inf)


def beam_select(beam_logp, cand_ids, cand_logp, Bout):
    """beam_logp [U, Bm] fp32, cand_ids int64 / cand_logp fp32 [U * Bm, C] -> (parent int32, item int64, logp fp32, step_logp fp32), each
    [U, Bout]: the live entries by (total descending with -0.0 as +0.0, beam ascending, candidate ascending); total is ONE fp32 add."""
    beam_logp = np.asarray(beam_logp, F32)
    cand_ids = np.asarray(cand_ids, np.int64)
    cand_logp = np.asarray(cand_logp, F32)
    U, Bm = beam_logp.shape
    C = cand_ids.shape[1]
    parent = np.full((U, Bout), -1, np.int32)
    item = np.full((U, Bout), -1, np.int64)
    logp = np.full((U, Bout), NEG_INF, F32)
    step = np.full((U, Bout), NEG_INF, F32)
    with np.errstate(over="ignore", invalid="ignore"):
        for u in range(U):
            entries = []
            for b in range(Bm):
                bl = beam_logp[u, b]
                if not bl > NEG_INF:
                    continue
                for c in range(C):
                    cl = cand_logp[u * Bm + b, c]
                    if cand_ids[u * Bm + b, c] < 0 or not cl > NEG_INF:
                        continue
                    total = F32(bl + cl)                                   # both operands are fp32: one rounded fp32 add
                    key = F32(0.0) if total == 0 else total                # -0.0 counts as +0.0
                    entries.append((-float(key), b, c, total))
            entries.sort(key=lambda e: e[:3])
            for t, (_, b, c, total) in enumerate(entries[:Bout]):
                parent[u, t], item[u, t], logp[u, t], step[u, t] = b, cand_ids[u * Bm + b, c], total, cand_logp[u * Bm + b, c]
    return parent, item, logp, step


def advance(tokens_in, len_in, exclude_in, path_in, path_logp_in, parent, item, item_logp, G_in, G_out, P, T, V, first_item, mask_id, t,
            ex_col):
    """The next step's rows.  Returns a dict: tokens / mask [N_out, L] int64, len [N_out] int32, positions [N_out, P] int64, exclude
    [N_out, E] int64, path [N_out, T] int64, path_logp [N_out, T] fp32.  parent None: row n continues row n.  path_in / path_logp_in
    None: all -1 / all -inf.  item_logp None: path_logp is not formed (None)."""
    tokens_in = np.asarray(tokens_in, np.int64)
    N_in, L = tokens_in.shape
    item = np.asarray(item, np.int64)
    N_out = item.shape[0]
    E = exclude_in.shape[1]
    assert N_in % G_in == 0 and N_out % G_out == 0 and N_in // G_in == N_out // G_out and (parent is not None or G_in == G_out)
    out = dict(tokens=np.zeros((N_out, L), np.int64), mask=np.zeros((N_out, L), np.int64), len=np.zeros(N_out, np.int32),
               positions=np.zeros((N_out, P), np.int64), exclude=np.zeros((N_out, E), np.int64), path=np.full((N_out, T), -1, np.int64),
               path_logp=None if item_logp is None else np.full((N_out, T), NEG_INF, F32))
    for n in range(N_out):
        group0 = n // G_out * G_in
        par = n % G_out if parent is None else int(parent[n])
        live = 0 <= par < G_in and first_item <= item[n] < V
        s = group0 + par if live else group0
        ln = int(min(max(int(len_in[s]), 1), L))
        row = tokens_in[s].copy()
        if live:
            if ln < L:
                row[ln - 1] = item[n]
                row[ln] = mask_id
                row[ln + 1:] = 0
                ln += 1
            else:
                row[:L - 2] = tokens_in[s][1:L - 1]
                row[L - 2] = item[n]
                row[L - 1] = mask_id
        out["tokens"][n] = row
        out["mask"][n, :ln] = 1
        out["len"][n] = ln
        out["positions"][n, 0] = ln - 1
        out["exclude"][n] = exclude_in[s]
        if live:
            out["exclude"][n, ex_col] = item[n]
            if path_in is not None:
                out["path"][n] = path_in[s]
            out["path"][n, t] = item[n]
            if item_logp is not None:
                if path_logp_in is not None:
                    out["path_logp"][n] = path_logp_in[s]
                out["path_logp"][n, t] = item_logp[n]
    return out
