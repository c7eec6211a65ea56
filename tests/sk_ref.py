"""numpy reference of the shell-averaged structure factor (pde_opt_amd.structure_factor, csrc/structure_factor.hip;
DESIGN.md section 4.20), on ``np.fft.rfftn`` in fp64.  Independent of the package: it takes ``points`` and box lengths.

    dk = max_a(2 pi / L_a);   t_a[i] = (2 pi fftfreq(n_a, L_a / n_a)[i] / dk)^2
    b  = floor(sqrt(q) + 0.5),  q = t_0[i] + t_1[m]  or  (t_0[i] + t_1[j]) + t_2[m]  on the half spectrum of rfftn
    w  = 1 for m = 0 and (n_last even) m = n_last / 2, else 2;  0 for the zero mode
    P_b = sum_shell w |u^|^2;  counts_b = sum_shell w;  S_b = P_b / (counts_b N);  k_b = b dk
    variance = sum P_b / N^2;  k1 = sum k S / sum S;  k2 = sqrt(sum k^2 S / sum S);  length = 2 pi / k1
"""
import numpy as np

GRIDS = [((37, 130), (1.0, 1.0)), ((24, 33), (1.0, 1.7)), ((64, 64), (1.0, 1.0)), ((12, 10, 18), (1.0, 1.0, 1.0)),
         ((9, 16, 34), (1.0, 0.8, 1.3))]


def white_noise(points, batch, seed):
    """``0.5 + 0.1 standard_normal``: broadband, every shell populated, a large zero mode"""
    return 0.5 + 0.1 * np.random.default_rng(seed).standard_normal((batch,) + tuple(points))


def tables(points, lengths):
    dk = max(2.0 * np.pi / v for v in lengths)
    return tuple((2.0 * np.pi * np.fft.fftfreq(n, v / n) / dk) ** 2 for n, v in zip(points, lengths)), dk


def n_bins_of(tabs):
    q = tabs[0].max()
    for t in tabs[1:]:
        q = q + t.max()
    return 1 + int(np.floor(np.sqrt(q) + 0.5))


def half_bins(points, lengths):
    """shell index and hermitian weight of every mode of the half spectrum, the shell count, dk"""
    tabs, dk = tables(points, lengths)
    nh = points[-1] // 2 + 1
    if len(points) == 2:
        q = tabs[0][:, None] + tabs[1][None, :nh]
    else:
        q = (tabs[0][:, None, None] + tabs[1][None, :, None]) + tabs[2][None, None, :nh]
    b = np.floor(np.sqrt(q) + 0.5).astype(np.int64)
    w = np.full(q.shape, 2.0)
    w[..., 0] = 1.0
    if points[-1] % 2 == 0:
        w[..., nh - 1] = 1.0
    w[(0,) * len(points)] = 0.0
    return b, w, n_bins_of(tabs), dk


def full_bins(points, lengths):
    """the same shells on the full spectrum of fftn, every mode with weight 1 but the zero mode"""
    tabs, _ = tables(points, lengths)
    if len(points) == 2:
        q = tabs[0][:, None] + tabs[1][None, :]
    else:
        q = (tabs[0][:, None, None] + tabs[1][None, :, None]) + tabs[2][None, None, :]
    w = np.ones(q.shape)
    w[(0,) * len(points)] = 0.0
    return np.floor(np.sqrt(q) + 0.5).astype(np.int64), w


def shell_sums(power_half, b, w, n_bins):
    """``P_b`` of a batch of half-spectrum powers ``|u^|^2`` (fp64), shape (B, n_bins)"""
    return np.stack([np.bincount(b.ravel(), weights=(w * p).ravel(), minlength=n_bins) for p in power_half])


def power(u, lengths):
    """(P (B, n_bins), counts (n_bins,), dk) of a batch ``u`` (B, *points), the transform in fp64"""
    u = np.asarray(u, dtype=np.float64)
    points = u.shape[1:]
    b, w, n_bins, dk = half_bins(points, lengths)
    uh = np.fft.rfftn(u, axes=tuple(range(1, u.ndim)))
    p = shell_sums(uh.real**2 + uh.imag**2, b, w, n_bins)
    return p, np.bincount(b.ravel(), weights=w.ravel(), minlength=n_bins), dk


def power_full(u, lengths):
    """the same sums from the full ``fftn``"""
    u = np.asarray(u, dtype=np.float64)
    points = u.shape[1:]
    b, w = full_bins(points, lengths)
    n_bins = n_bins_of(tables(points, lengths)[0])
    uf = np.fft.fftn(u, axes=tuple(range(1, u.ndim)))
    return shell_sums(uf.real**2 + uf.imag**2, b, w, n_bins), np.bincount(b.ravel(), weights=w.ravel(), minlength=n_bins)


def derived(p, counts, n, dk):
    """dict of s, k, variance, k1, k2, length from shell sums ``p`` (..., n_bins)"""
    k = np.arange(len(counts)) * dk
    s = np.zeros_like(p)
    nz = counts > 0
    s[..., nz] = p[..., nz] / (counts[nz] * n)
    tot = s.sum(axis=-1)
    k1 = (k * s).sum(axis=-1) / tot
    return dict(s=s, k=k, variance=p.sum(axis=-1) / float(n) ** 2, k1=k1, k2=np.sqrt((k**2 * s).sum(axis=-1) / tot),
                length=2.0 * np.pi / k1)


def plane_wave(points=(32, 48)):
    """``0.3 + 0.2 cos(2 pi (3 x + 4 y))`` on the unit box at the cells' mid-points: all of N^2 0.02 in shell 5"""
    x = (np.arange(points[0]) + 0.5) / points[0]
    y = (np.arange(points[1]) + 0.5) / points[1]
    return 0.3 + 0.2 * np.cos(2.0 * np.pi * (3.0 * x[:, None] + 4.0 * y[None, :]))
