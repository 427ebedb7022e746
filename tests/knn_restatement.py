"""Brute-force CPU restatement of ``fg_knn`` (a helper, not a test): the same fp32 arithmetic, candidate by candidate,
so that the kernel's distances AND its choice among ties can be compared bit for bit.

    dx = xq - xp (y, z alike), d2 = (dx dx + dy dy) + dz dz   -- each operation rounded to fp32, nothing fused
    candidates ordered by (d2, row number), the query's own row excluded by number

d2 is non-negative, so its int32 bit pattern orders like its value; the k best are the k smallest composite keys
(bits of d2) << 32 | row."""
import torch


def knn_restatement(x: torch.Tensor, k: int, rows: int = 1024):
    """x [N,3] -> (d2 [N,k] float32 ascending, idx [N,k] int32), N > k."""
    x = x.detach().cpu().float().contiguous()
    n = x.shape[0]
    assert n > k >= 1
    xs, ys, zs = x[:, 0].contiguous(), x[:, 1].contiguous(), x[:, 2].contiguous()
    col = torch.arange(n, dtype=torch.int64)
    d2_out = torch.empty(n, k, dtype=torch.float32)
    idx_out = torch.empty(n, k, dtype=torch.int32)
    self_key = torch.iinfo(torch.int64).max
    for i in range(0, n, rows):
        dx = xs[i : i + rows, None] - xs[None, :]
        dy = ys[i : i + rows, None] - ys[None, :]
        dz = zs[i : i + rows, None] - zs[None, :]
        d2 = (dx * dx + dy * dy) + dz * dz
        key = (d2.view(torch.int32).to(torch.int64) << 32) | col[None, :]
        m = key.shape[0]
        key[torch.arange(m), torch.arange(i, i + m)] = self_key
        best = key.topk(k, dim=1, largest=False, sorted=True).values
        d2_out[i : i + m] = (best >> 32).to(torch.int32).view(torch.float32)
        idx_out[i : i + m] = (best & 0xFFFFFFFF).to(torch.int32)
    return d2_out, idx_out
