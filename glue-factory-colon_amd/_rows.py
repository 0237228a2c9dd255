"""Row plumbing of the LightGlue modules (`lightglue.py`, `lightglue_training.py`): the two sides of a uniform batch as
one [B*M + B*N, C] row buffer (side 0 first, the layout the library reads) and back, and the match outputs of one batch.
Tensor views and allocations only; nothing here launches a kernel of the library or imports the package."""
import torch


def pack_sides(a, b):
    """[B,M,C] and [B,N,C] -> [B*M + B*N, C] rows (side 0 first).  A view when `b` starts where `a` ends in the same
    allocation (both views extracted by one call), a concatenation otherwise."""
    c = a.shape[-1]
    ra, rb = a.numel() // c, b.numel() // c
    if (a.is_contiguous() and b.is_contiguous() and a.dtype == b.dtype == torch.float32
            and b.data_ptr() == a.data_ptr() + a.numel() * 4
            and a.untyped_storage().data_ptr() == b.untyped_storage().data_ptr()):
        return a.as_strided((ra + rb, c), (c, 1))
    return torch.cat([a.reshape(ra, c), b.reshape(rb, c)], 0)


def split_sides(t, b, m, n):
    """The inverse of `pack_sides`: [..., B*M + B*N, C] -> views [..., B, M, C] and [..., B, N, C]."""
    lead, c = t.shape[:-2], t.shape[-1]
    return t[..., :b * m, :].view(*lead, b, m, c), t[..., b * m:, :].view(*lead, b, n, c)


def stacked_sides(stack, b, m, n):
    """The row buffers of L layers [L, B*M + B*N, C] as the per-pair tensors [B, L, M, C] and [B, L, N, C]: permuted
    views, no transposing copy."""
    s0, s1 = split_sides(stack, b, m, n)
    return s0.permute(1, 0, 2, 3), s1.permute(1, 0, 2, 3)


def put_sides(out, key, sides):
    """out[key + "0"], out[key + "1"] = the two sides."""
    out[key + "0"], out[key + "1"] = sides


def match_outputs(b, m, n, device):
    """Uninitialised matches0 [B,M], matches1 [B,N] (int64), matching_scores0 / 1 (float32) and the log assignment
    [B, M+1, N+1]: the library writes every element of them."""
    return (torch.empty((b, m), device=device, dtype=torch.long), torch.empty((b, n), device=device, dtype=torch.long),
            torch.empty((b, m), device=device), torch.empty((b, n), device=device),
            torch.empty((b, m + 1, n + 1), device=device))
