"""fp64 torch reference of compact bilinear pooling and of the MCB attention / head built on it, written from the
formulas of include/fvta_hip.h (nothing here is the library's or the reference project's code).

  z[r,k] = sum over (i,j) with (h1[i] + h2[j]) mod D = k of  s1[i] s2[j] x[r,i] q[n(r),j],   n(r) = r // P

`cbp_direct` is that definition; `cbp_fft` is the route the layer itself takes (two count sketches, FFT, product,
inverse FFT, real part).  `normalize` is l2_normalize(sqrt(sign(z) z)) with the library's zero convention: the square
root's derivative is taken as 0 at z = 0, and a row of zeros gives zeros."""
import torch


def _t(a, dtype):
    return a.to(dtype) if torch.is_tensor(a) else torch.as_tensor(a, dtype=dtype)


def _tables(h1, s1, h2, s2):
    return _t(h1, torch.int64), _t(s1, torch.float64), _t(h2, torch.int64), _t(s2, torch.float64)


def cbp_terms(x, q, h1, s1, h2, s2, D, P=1):
    """(bucket index of every (i,j) [d1*d2], the terms s1 s2 x q [R, d1*d2])"""
    h1, s1, h2, s2 = _tables(h1, s1, h2, s2)
    qr = q.repeat_interleave(int(P), 0)                                # [R,d2]
    terms = (x * s1)[:, :, None] * (qr * s2)[:, None, :]               # [R,d1,d2]
    bucket = (h1[:, None] + h2[None, :]) % int(D)
    return bucket.reshape(-1), terms.reshape(x.shape[0], -1)


def cbp_direct(x, q, h1, s1, h2, s2, D, P=1):
    """x [R,d1], q [R/P,d2] (fp64) -> z [R,D] by the definition"""
    bucket, terms = cbp_terms(x, q, h1, s1, h2, s2, D, P)
    return torch.zeros(x.shape[0], int(D), dtype=x.dtype).index_add(1, bucket, terms)


def cbp_abs_terms(x, q, h1, s1, h2, s2, D, P=1):
    """sum of |terms| per bucket [R,D]: the scale a bucket's rounding error lives on"""
    bucket, terms = cbp_terms(x, q, h1, s1, h2, s2, D, P)
    return torch.zeros(x.shape[0], int(D), dtype=x.dtype).index_add(1, bucket, terms.abs())


def cbp_fft(x, q, h1, s1, h2, s2, D, P=1):
    """the layer's own route: index_add sketches, fft, product, ifft, real part"""
    h1, s1, h2, s2 = _tables(h1, s1, h2, s2)
    R = x.shape[0]
    sk1 = torch.zeros(R, int(D), dtype=x.dtype).index_add(1, h1, x * s1)
    sk2 = torch.zeros(R, int(D), dtype=x.dtype).index_add(1, h2, q.repeat_interleave(int(P), 0) * s2)
    return torch.fft.ifft(torch.fft.fft(sk1) * torch.fft.fft(sk2)).real


def normalize(z):
    """y = w rsqrt(max(sum w^2, 1e-12)), w = sqrt|z|; autograd gives d w / d z = 0 at z = 0"""
    nz = z != 0
    w = torch.where(nz, z.abs(), torch.ones_like(z)).sqrt() * nz
    return w * torch.rsqrt(torch.clamp((w * w).sum(-1, keepdim=True), min=1e-12))


def mcb_attention(hpis, gq, tables, filter_conv1, filter_conv2):
    """hpis [N,M,JI,idim], gq [N,qdim] -> (attended [N,idim], att [N,M*JI]): pooled and normalised rows, relu(linear)
    twice without a bias, a softmax over all positions, the weighted sum of the photo rows"""
    N, M, JI, idim = hpis.shape
    T = M * JI
    D = filter_conv1.shape[0]
    g = normalize(cbp_direct(hpis.reshape(N * T, idim), gq, *tables, D, P=T))
    c2 = torch.relu(torch.relu(g @ filter_conv1) @ filter_conv2)
    att = torch.softmax(c2.reshape(N, T), 1)
    return (hpis.reshape(N, T, idim) * att[:, :, None]).sum(1), att


def mcb_head(lq, g1, hpis, lchoices, tables, filter_conv1, filter_conv2, Wt, bt, Wo, bo, add_tanh=False):
    """-> (logits [N,C], att): the attended photo row through a linear to the question's width, then one linear over
    concat([gq, g1, g_mcb, gch, gq*g1, gq*g_mcb, gq*gch]) per choice"""
    act = torch.tanh if add_tanh else (lambda t: t)
    attended, att = mcb_attention(hpis, lq, tables, filter_conv1, filter_conv2)
    g_mcb = act(attended @ Wt + bt)
    C = lchoices.shape[1]
    tile = lambda t: t[:, None, :].expand(-1, C, -1)
    q_t, g1_t, m_t = tile(lq), tile(g1), tile(g_mcb)
    cat = torch.cat([q_t, g1_t, m_t, lchoices, q_t * g1_t, q_t * m_t, q_t * lchoices], 2)
    return act(cat @ Wo + bo).squeeze(2), att
