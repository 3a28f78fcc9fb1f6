"""The torch reference of fvta_gru_seq (a helper, not a test): TensorFlow 1's GRUCell under dynamic_rnn(sequence_length),
written from the formulas of include/fvta_hip.h with the literal concats, in whatever dtype the inputs have (the tests pass
fp64 leaves and differentiate it with autograd).

    v  = sigmoid([x_t, h] . Wg + bg)      r = v[:, :d], u = v[:, d:]
    c  = tanh([x_t, r * h] . Wc + bc)
    h' = u * h + (1 - u) * c

Lengths and `reverse` are implemented by indexing per row: row n takes its steps over positions 0 .. lens[n]-1 (reverse:
lens[n]-1 .. 0), out[n, t] is the state after the step at position t, the positions t >= lens[n] stay zero, and h_last[n] is
the state after the row's last step (h0[n], or zero, for an empty row)."""
import torch


def gru_cell(x, h, Wg, bg, Wc, bc):
    d = h.shape[1]
    v = torch.sigmoid(torch.cat([x, h], 1) @ Wg + bg)
    r, u = v[:, :d], v[:, d:]
    c = torch.tanh(torch.cat([x, r * h], 1) @ Wc + bc)
    return u * h + (1 - u) * c


def gru_seq(x, lens, h0, Wg, bg, Wc, bc, reverse=False):
    """x [N,T,in], lens (N ints) or None, h0 [N,d] or None -> (out [N,T,d], h_last [N,d])"""
    N, T, _ = x.shape
    d = Wc.shape[1]
    lens = [T] * N if lens is None else [int(v) for v in lens]
    outs, lasts = [], []
    for n in range(N):
        h = h0[n:n + 1] if h0 is not None else torch.zeros(1, d, dtype=x.dtype)
        rows = [torch.zeros(1, d, dtype=x.dtype) for _ in range(T)]
        for t in (range(lens[n] - 1, -1, -1) if reverse else range(lens[n])):
            h = gru_cell(x[n:n + 1, t], h, Wg, bg, Wc, bc)
            rows[t] = h
        outs.append(torch.cat(rows, 0))
        lasts.append(h)
    return torch.stack(outs, 0), torch.cat(lasts, 0)


def flip_prefix(x, lens):
    """every row's valid prefix reversed in place of itself, the padding left where it is"""
    y = x.clone()
    for n, L in enumerate(int(v) for v in lens):
        y[n, :L] = x[n, :L].flip(0)
    return y


def bigru_sum(f_in, lens, fw, bw):
    """model_dmnplus.py:478-486: the forward and the backward GRU's outputs summed; fw / bw = (Wg, bg, Wc, bc)"""
    return gru_seq(f_in, lens, None, *fw)[0] + gru_seq(f_in, lens, None, *bw, reverse=True)[0]
