"""float64 restatement of the evaluation kernel (csrc/loss.hip, vitamd_classify_metrics), the comparison its GPU tests use, and the
planted mistakes the host test proves that comparison against.  No GPU, no library: plain torch on the CPU.

rank[r] = the number of columns v != t that rank above the target t of row r, where v ranks above t unless x_v < x_t, or x_v == x_t and
v > t (a NaN compares false).  Ignored rows: rank -1, loss 0, counted nowhere.  A target outside [0, V) that is not ignore_index: a
counted row of rank V and NaN loss."""
import torch

import _lm_ref as LR

F64 = torch.float64

BUGS = ("ties_ge", "ties_all_columns", "topk_le", "ignored_in_rows", "ignored_in_loss", "oor_skipped", "nan_target_correct")
ACC_BUGS = ("overwrite", "mean_per_call")


def metrics_ref(logits, target, topk, ignore_index=-100, bug=None):
    """logits [M, V] (any float dtype, compared and summed as stored, in float64), target int64 [M] -> dict: rank int64 [M], loss_row
    and lse float64 [M], counts = [rows, top-1 hits, top-k hits], loss_sum (Python float), valid bool [M].  bug: one of BUGS."""
    x = logits.to(F64)
    M, V = x.shape
    col = torch.arange(V)[None, :]
    ignored = target == ignore_index
    in_range = (target >= 0) & (target < V) & ~ignored
    oor = ~in_range & ~ignored
    if bug == "oor_skipped":
        ignored, oor = ignored | oor, torch.zeros_like(oor)
    tcol = torch.where(in_range, target, torch.zeros_like(target))[:, None]
    xt = x.gather(1, tcol)
    xt = torch.where(in_range[:, None], xt, torch.full_like(xt, float("nan")))
    below = (x < xt) | ((x == xt) & (col > tcol))
    if bug == "ties_ge":
        above = x >= xt
    elif bug == "ties_all_columns":
        above = ~(x < xt)
    else:
        above = ~below
    rank = (above & (col != tcol)).sum(dim=1)
    rank = torch.where(oor, torch.full_like(rank, V), rank)
    if bug == "nan_target_correct":
        rank = torch.where(in_range & torch.isnan(xt[:, 0]), torch.zeros_like(rank), rank)
    rank = torch.where(ignored, torch.full_like(rank, -1), rank)
    m = x.max(dim=-1, keepdim=True).values
    lse = (m + (x - m).exp().sum(dim=-1, keepdim=True).log()).squeeze(1)
    loss_row = lse - xt[:, 0]                                   # NaN where the target is out of range
    if bug == "ignored_in_loss":
        loss_row = torch.where(ignored, lse - x[:, 0], loss_row)
    else:
        loss_row = torch.where(ignored, torch.zeros_like(loss_row), loss_row)
    valid = rank >= 0
    rows = M if bug == "ignored_in_rows" else int(valid.sum())
    hit_k = (rank <= topk) if bug == "topk_le" else (rank < topk)
    counts = [rows, int((valid & (rank == 0)).sum()), int((valid & hit_k).sum())]
    loss_sum = float(loss_row.sum() if bug == "ignored_in_loss" else loss_row[valid].sum())
    return {"rank": rank, "loss_row": loss_row, "lse": lse, "counts": counts, "loss_sum": loss_sum, "valid": valid}


def accumulate(results, bug=None):
    """what an accumulator holds after the calls whose metrics_ref results are given, in order -> {"counts", "loss_sum"}.  bug: one of
    ACC_BUGS."""
    counts, loss_sum = [0, 0, 0], 0.0
    for r in results:
        add = r["loss_sum"] / max(r["counts"][0], 1) if bug == "mean_per_call" else r["loss_sum"]
        if bug == "overwrite":
            counts, loss_sum = list(r["counts"]), add
        else:
            counts, loss_sum = [a + b for a, b in zip(counts, r["counts"])], loss_sum + add
    return {"counts": counts, "loss_sum": loss_sum}


def row_bound(logits, target, ignore_index=-100):
    """the per-row bound of tests/_lm_ref.py::check_cross_entropy for this input, taken as it is: max(4 x torch fp32's own distance from
    float64 on loss_row, the floor), in units of max(1, |lse_ref|)"""
    ref = LR.cross_entropy_ref(logits, target, ignore_index)
    t32 = LR.cross_entropy_torch32(logits, target, ignore_index)
    return LR.bound(LR.cross_entropy_errors({"loss_row": t32["loss_row"]}, ref)["loss_row"])


def sum_allowance(ref, bound):
    """|loss_sum - sum_ref| may reach the sum over the counted rows of bound * max(1, |lse_ref|)"""
    return float((bound * ref["lse"][ref["valid"]].abs().clamp_min(1.0)).sum())


def check_metrics(got, ref, allowance, label=""):
    """The comparison of the GPU tests -> list of failure strings.  got: {"counts": 3 integers, "loss_sum": float, "rank": optional
    integer tensor [M]}; ref: a metrics_ref (or accumulate) result; allowance: what |loss_sum - ref| may reach (sum_allowance).  Integers
    must be equal.  A non-finite reference sum demands a non-finite sum of the same kind (NaN / +inf / -inf), never a number."""
    fails = []
    if "rank" in got and "rank" in ref and not torch.equal(got["rank"].to(torch.int64).cpu(), ref["rank"]):
        bad = (got["rank"].to(torch.int64).cpu() != ref["rank"]).nonzero().reshape(-1)
        r = int(bad[0])
        fails.append(f"{label} rank: {bad.numel()} rows differ, first row {r}: got {int(got['rank'][r])}, reference {int(ref['rank'][r])}")
    if [int(v) for v in got["counts"]] != list(ref["counts"]):
        fails.append(f"{label} counts: got {[int(v) for v in got['counts']]}, reference {list(ref['counts'])}")
    g, r = float(got["loss_sum"]), float(ref["loss_sum"])
    if r != r or r in (float("inf"), float("-inf")):
        if not (g != g if r != r else g == r):
            fails.append(f"{label} loss_sum: got {g!r}, reference {r!r}")
    else:
        print(f"{label} loss_sum: |{g!r} - {r!r}| = {abs(g - r):.3e} (allowed {allowance:.3e})")
        if not abs(g - r) <= allowance:
            fails.append(f"{label} loss_sum: |{g!r} - {r!r}| = {abs(g - r):.3e} > {allowance:.3e}")
    return fails
