"""Device reductions of the likelihood side: thin wrappers of efd_loglike / efd_inner_product /
efd_fisher_gram / efd_overlap_rows / efd_pair_stats / efd_td_split_pair_stats, and of the noise
realisations' efd_noise_fd / efd_noise_overlap_rows.

All run in libemrifd.so (HIP, gfx950) as fixed-partition two-pass reductions, so results are
bitwise reproducible. They read the channels in place: h, d complex128 [nchan][nbin], w float64
[nchan][nbin] (all contiguous, on one device); the result stays on the device until the caller
asks for it, so a batch of walkers costs one host synchronisation. fisher_gram takes the rows of
a Fisher matrix's stencil points and returns the whole [nparam][nparam] matrix from one pass;
overlap_rows takes many rows and one fixed waveform and returns every row's products with it.
"""

import ctypes

import numpy as _np

from . import _lib
from .summation import require_gpu


class Reducer:
    """Per-device scratch + entry points (one instance per device/stream user)."""

    def __init__(self, device=None):
        self.torch = torch = require_gpu()
        self.lib = _lib.load()
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None \
            else torch.device(device)
        self._scr_ll = torch.empty(_lib.EFD_LOGLIKE_SCRATCH, dtype=torch.float64,
                                   device=self.device)
        self._scr_ip = torch.empty(_lib.EFD_INNER_SCRATCH, dtype=torch.float64,
                                   device=self.device)

    def _stream(self):
        return ctypes.c_void_p(self.torch.cuda.current_stream(self.device).cuda_stream)

    def _check(self, x, name, dtype, shape):
        torch = self.torch
        if x.dtype != dtype or not x.is_contiguous() or x.device != self.device:
            raise ValueError(f"{name}: expected contiguous {dtype} on {self.device}, got "
                             f"{x.dtype} on {x.device}")
        if tuple(x.shape) != tuple(shape):
            raise ValueError(f"{name}: expected shape {tuple(shape)}, got {tuple(x.shape)}")
        return torch.view_as_real(x).data_ptr() if x.is_complex() else x.data_ptr()

    def _rows(self, x, msg, dim=None, nrow=None, nelem=None):
        """(pointer, stride in complex elements, row count, elements per row) of the rows of a
        complex128 matrix on this device: each row contiguous, the rows a fixed stride apart and
        not overlapping. A row is x[r] whole, or with nelem given the first nelem elements of a
        2-D x's row. dim, nrow: x's dimensions and row count where the caller fixes them.
        ValueError(msg) where x is no such matrix, "<name>: ... overlapping rows" (the name is
        msg's) where its rows overlap."""
        torch = self.torch
        if (x.dtype != torch.complex128 or x.device != self.device
                or (x.dim() < 2 if dim is None else x.dim() != dim)
                or (x.shape[0] < 1 if nrow is None else x.shape[0] != nrow)
                or (not x[0].is_contiguous() if nelem is None
                    else x.shape[1] < nelem or x.stride(1) != 1)):
            raise ValueError(msg)
        whole = nelem is None
        nelem = int(x[0].numel()) if whole else nelem
        stride = int(x.stride(0)) if x.shape[0] > 1 else nelem
        if stride < nelem or (whole and nelem == 0):
            raise ValueError(f"{msg.split(':')[0]}: {'empty or ' if whole else ''}overlapping rows")
        return torch.view_as_real(x).data_ptr(), stride, int(x.shape[0]), nelem

    def _scratch(self, name, size):
        """The float64 scratch tensor `name` of `size` doubles, allocated at its first use."""
        scr = getattr(self, name, None)
        if scr is None:
            scr = self.torch.empty(size, dtype=self.torch.float64, device=self.device)
            setattr(self, name, scr)
        return scr

    def loglike(self, h, d, w, out=None):
        """-1/2 * 4 * sum |d - h w|^2 over all channels and bins (likelihood.py:257-274).

        h may be None (data-only term). Returns a 1-element float64 device tensor (or writes
        into `out`, a 1-element view, e.g. one slot of a batch result).
        """
        torch = self.torch
        nchan, nbin = int(d.shape[0]), int(d.shape[1])
        pd = self._check(d, "d", torch.complex128, (nchan, nbin))
        pw = self._check(w, "w", torch.float64, (nchan, nbin))
        ph = None if h is None else self._check(h, "h", torch.complex128, (nchan, nbin))
        if out is None:
            out = torch.empty(1, dtype=torch.float64, device=self.device)
        _lib.check(self.lib.efd_loglike(ph, pd, pw, nchan, nbin, out.data_ptr(),
                                        self._scr_ll.data_ptr(), self._stream()),
                   "efd_loglike", self.lib)
        return out

    def inner(self, a, b, w=None):
        """4 * sum conj(a) b w as a complex128 device scalar (diagnostic.py:95-110)."""
        torch = self.torch
        nchan, nbin = int(a.shape[0]), int(a.shape[1])
        pa = self._check(a, "a", torch.complex128, (nchan, nbin))
        pb = self._check(b, "b", torch.complex128, (nchan, nbin))
        pw = None if w is None else self._check(w, "w", torch.float64, (nchan, nbin))
        out = torch.empty(1, dtype=torch.complex128, device=self.device)
        _lib.check(self.lib.efd_inner_product(pa, pb, pw, nchan, nbin,
                                              torch.view_as_real(out).data_ptr(),
                                              self._scr_ip.data_ptr(), self._stream()),
                   "efd_inner_product", self.lib)
        return out

    def fisher_gram(self, rows, coef, w, npoint, dh=None):
        """gram[i][j] = 4 sum_e w[e] Re(conj(D_i[e]) D_j[e]), D_i = sum_s coef[i][s] rows[i npoint
        + s], as a float64 [nparam][nparam] device tensor (efd_fisher_gram: one pass, the stencil
        applied per element before the products; lisatools fisher's reduction,
        diagnostic.py:353-381).

        rows: complex128 [nparam * npoint][...]: every row's trailing dimensions contiguous
        (nelem elements), rows a fixed stride apart (a slice of a wider buffer is fine);
        coef: host [nparam][npoint]; w: float64 with nelem elements on the device, or None
        (w = 1); dh: None, or a contiguous complex128 [nparam][...] tensor that receives D.
        """
        torch = self.torch
        if npoint not in (1, 2, 4):
            raise ValueError("npoint must be 1, 2 or 4")
        coef = _np.ascontiguousarray(coef, dtype=_np.float64)
        if coef.ndim != 2 or coef.shape[1] != npoint:
            raise ValueError(f"coef: expected [nparam][{npoint}], got {coef.shape}")
        nparam = int(coef.shape[0])
        if not 1 <= nparam <= _lib.EFD_FISHER_MAX_PARAMS:
            raise ValueError(f"nparam must be in 1..{_lib.EFD_FISHER_MAX_PARAMS}")
        prows, stride, _, nelem = self._rows(
            rows, f"rows: expected complex128 [{nparam * npoint}][...] on {self.device} with "
            "contiguous rows", nrow=nparam * npoint)
        pw = None
        if w is not None:
            if w.numel() != nelem:
                raise ValueError(f"w: expected {nelem} elements, got {w.numel()}")
            pw = self._check(w, "w", torch.float64, tuple(w.shape))
        pdh = None
        if dh is not None:
            if dh.numel() != nparam * nelem or dh.shape[0] != nparam:
                raise ValueError(f"dh: expected [{nparam}][...] with {nelem} elements a row")
            pdh = self._check(dh, "dh", torch.complex128, tuple(dh.shape))
        scr = self._scratch("_scr_fg", _lib.EFD_FISHER_SCRATCH)
        gram = torch.empty((nparam, nparam), dtype=torch.float64, device=self.device)
        _lib.check(self.lib.efd_fisher_gram(prows, stride, nparam, npoint, coef.ctypes.data, pw,
                                            nelem, pdh, gram.data_ptr(), scr.data_ptr(),
                                            self._stream()),
                   "efd_fisher_gram", self.lib)
        return gram

    def overlap_rows(self, rows, t, u=None, w=None):
        """Every row's overlap with one fixed waveform r = t - u (u None: r = t) in one pass
        (efd_overlap_rows; the reduction of lisatools' mismatch_criterion, diagnostic.py:622-638,
        and of cutler_vallisneri_bias, :812-823): (out, rr) with out float64 [nrow][3] =
        4 sum_e w (Re conj(h_k) r, Im conj(h_k) r, |h_k|^2) and rr = 4 sum_e w |r|^2 a 0-d
        tensor, both views of one device tensor of 3 nrow + 1 doubles (overlap_rows_flat returns
        that one: a single host transfer brings everything back).

        rows: complex128 [nrow][...] as fisher_gram's (contiguous rows a fixed stride apart);
        t, u: contiguous complex128 with a row's nelem elements; w: float64 with nelem elements,
        or None (w = 1). More than EFD_OVERLAP_MAX_ROWS rows go in several calls; a row's numbers
        are bitwise what any other split gives (the kernel's subset promise).
        """
        res = self.overlap_rows_flat(rows, t, u, w)
        nrow = int(rows.shape[0])
        return res[:3 * nrow].view(nrow, 3), res[3 * nrow]

    def overlap_rows_flat(self, rows, t, u=None, w=None):
        """overlap_rows' numbers as efd_overlap_rows lays them out: float64 [3 nrow + 1] on the
        device, (re, im, nn) per row and then rr."""
        torch = self.torch
        base, stride, nrow, nelem = self._rows(
            rows, f"rows: expected complex128 [nrow][...] on {self.device} with contiguous rows")
        ptrs = []
        for x, name, dtype in ((t, "t", torch.complex128), (u, "u", torch.complex128),
                               (w, "w", torch.float64)):
            if x is None:
                if name == "t":
                    raise ValueError("t: a complex128 tensor is required")
                ptrs.append(None)
                continue
            if x.numel() != nelem:
                raise ValueError(f"{name}: expected {nelem} elements, got {x.numel()}")
            ptrs.append(self._check(x, name, dtype, tuple(x.shape)))
        scr = self._scratch("_scr_ov", _lib.EFD_OVERLAP_SCRATCH)
        M = _lib.EFD_OVERLAP_MAX_ROWS
        ncall = (nrow + M - 1) // M
        # call c writes its 3 n + 1 doubles at 3 c M: its |r|^2 lands on the next call's first
        # slot and is overwritten by it, the last call's stays at 3 nrow
        res = torch.empty(3 * nrow + 1, dtype=torch.float64, device=self.device)
        for c in range(ncall):
            n = min(M, nrow - c * M)
            _lib.check(self.lib.efd_overlap_rows(base + 16 * stride * c * M, stride, n, *ptrs,
                                                 nelem, res.data_ptr() + 8 * 3 * c * M,
                                                 scr.data_ptr(), self._stream()),
                       "efd_overlap_rows", self.lib)
        return res

    def _pair_rows(self, x, name, nchan=None):
        """(pointer, stride in complex elements, nrow, nchan, nbin) of rows complex128
        [nrow][nchan][nbin]: every row contiguous, rows a fixed stride apart."""
        ptr, stride, nrow, _ = self._rows(
            x, f"{name}: expected complex128 [nrow][nchan][nbin] on {self.device} with "
            "contiguous rows", dim=3)
        nch, nbin = int(x.shape[1]), int(x.shape[2])
        if nch not in (1, 2) or (nchan is not None and nch != nchan):
            raise ValueError(f"{name}: expected {nchan or '1 or 2'} channels, got {nch}")
        return ptr, stride, nrow, nch, nbin

    def _pair_scratch(self):
        return self._scratch("_scr_ps", _lib.EFD_PAIR_SCRATCH)

    def _pair_out(self, out, nrow, nchan):
        torch = self.torch
        if out is None:
            return torch.empty((nrow, nchan, 5), dtype=torch.float64, device=self.device)
        self._check(out, "out", torch.float64, (nrow, nchan, 5))
        return out

    def pair_stats(self, a, b, w, out=None):
        """(aa, bb, abr, abi, dd) of every (a_r, b_r) pair and channel in one pass over each
        (efd_pair_stats; the mode-by-mode driver's inner products, check_mode_by_mode.py:292-326)
        as a float64 [nrow][nchan][5] device tensor: 4 sum_k w (|a|^2, |b|^2, Re conj(a) b,
        Im conj(a) b, |a - b|^2), the difference formed per element.

        a, b: complex128 [nrow][nchan][nbin], nchan 1 or 2, contiguous rows a fixed stride
        apart; w: float64 [nbin] shared by the channels and rows, or None (w = 1). More than
        EFD_PAIR_MAX_ROWS rows go in several calls; a row's numbers are bitwise what any other
        split gives."""
        torch = self.torch
        pa, sa, nrow, nchan, nbin = self._pair_rows(a, "a")
        pb, sb, nrb, _, nbb = self._pair_rows(b, "b", nchan)
        if (nrb, nbb) != (nrow, nbin):
            raise ValueError(f"b: expected shape {tuple(a.shape)}, got {tuple(b.shape)}")
        pw = None if w is None else self._check(w, "w", torch.float64, (nbin,))
        out = self._pair_out(out, nrow, nchan)
        scr = self._pair_scratch()
        M = _lib.EFD_PAIR_MAX_ROWS
        for r0 in range(0, nrow, M):
            n = min(M, nrow - r0)
            _lib.check(self.lib.efd_pair_stats(pa + 16 * sa * r0, sa, pb + 16 * sb * r0, sb, n,
                                               nchan, nbin, pw,
                                               out.data_ptr() + 8 * 5 * nchan * r0,
                                               scr.data_ptr(), self._stream()),
                       "efd_pair_stats", self.lib)
        return out

    def td_split_pair_stats(self, Z, n, gain, a, w, keep=None, out=None):
        """pair_stats with b_r = the two channels of row r of Z (efd_td_split's gain H+, gain Hx
        over the nb = (n + 1) // 2 positive-frequency bins), never stored
        (efd_td_split_pair_stats): float64 [rows][2][5] on the device.

        Z: complex128 [rows][>= n], natural-order transforms of w (h+ - i hx), rows a fixed
        stride apart; a: complex128 [rows][2][nb]; w: float64 [nb] or None; keep: uint8 [nb] or
        None (a dropped bin has b = 0)."""
        torch = self.torch
        n = int(n)
        msg = f"Z: expected complex128 [rows][>= {n}] on {self.device} with contiguous rows"
        if n < 1:
            raise ValueError(msg)
        pz, zs, rows, _ = self._rows(Z, msg, dim=2, nelem=n)
        nb = (n + 1) // 2
        pa, sa, nra, _, nba = self._pair_rows(a, "a", 2)
        if (nra, nba) != (rows, nb):
            raise ValueError(f"a: expected shape {(rows, 2, nb)}, got {tuple(a.shape)}")
        pw = None if w is None else self._check(w, "w", torch.float64, (nb,))
        pk = None if keep is None else self._check(keep, "keep", torch.uint8, (nb,))
        out = self._pair_out(out, rows, 2)
        scr = self._pair_scratch()
        M = _lib.EFD_PAIR_MAX_ROWS
        for r0 in range(0, rows, M):
            m = min(M, rows - r0)
            _lib.check(self.lib.efd_td_split_pair_stats(pz + 16 * zs * r0, zs, n, m, float(gain),
                                                        pa + 16 * sa * r0, sa, pw, pk,
                                                        out.data_ptr() + 8 * 10 * r0,
                                                        scr.data_ptr(), self._stream()),
                       "efd_td_split_pair_stats", self.lib)
        return out

    def dh_hh_rows(self, rows, d, w, out=None):
        """(Re <d|h_r>, Im <d|h_r>, <h_r|h_r>) of every written template row against one
        weighted data d and weight w (efd_dh_hh_rows; the fused mode sum's terms, see
        include/emrifd.h) as a float64 [nrow][3] device tensor.

        rows: complex128 [nrow][nchan][nbin] (or one template [nchan][nbin]), nchan 1 or 2,
        contiguous rows a fixed stride apart; d: complex128 [nchan][nbin]; w: float64
        [nchan][nbin]. More than EFD_DH_MAX_ROWS rows go in several calls; a row's numbers are
        bitwise what any other split gives."""
        torch = self.torch
        if rows.dim() == 2:
            rows = rows[None]
        ph, sh, nrow, nchan, nbin = self._pair_rows(rows, "rows")
        pd = self._check(d, "d", torch.complex128, (nchan, nbin))
        pw = self._check(w, "w", torch.float64, (nchan, nbin))
        if out is None:
            out = torch.empty((nrow, 3), dtype=torch.float64, device=self.device)
        elif out.dtype != torch.float64 or out.numel() < 3 * nrow or not out.is_contiguous():
            raise ValueError(f"dh_hh_rows: out float64 [{nrow}][3], contiguous")
        scr = self._scratch("_scr_dh", _lib.EFD_DH_SCRATCH)
        M = _lib.EFD_DH_MAX_ROWS
        for r0 in range(0, nrow, M):
            n = min(M, nrow - r0)
            _lib.check(self.lib.efd_dh_hh_rows(ph + 16 * sh * r0, sh, n, pd, pw, nchan, nbin,
                                               out.data_ptr() + 24 * r0, scr.data_ptr(),
                                               self._stream()),
                       "efd_dh_hh_rows", self.lib)
        return out

    def noise_fd(self, out, seed, realization=0, bin0=0, gain=None, accumulate=False):
        """out[c][i] = gain[c][i] * 0.5 * xi(c, bin0 + i) (efd_noise_fd; with accumulate added
        to out): the counter-based draws of include/emrifd.h's "Noise realisations", a function
        of (seed, realization, channel, bin) alone. out: complex128 [nchan][nbin] on this
        device; gain: float64 [nchan][nbin] or None (= 1), a gain of 0 or NaN leaves the bin
        without noise. Returns out."""
        torch = self.torch
        if out.dim() != 2:
            raise ValueError(f"out: expected complex128 [nchan][nbin], got {tuple(out.shape)}")
        nchan, nbin = int(out.shape[0]), int(out.shape[1])
        po = self._check(out, "out", torch.complex128, (nchan, nbin))
        pg = None if gain is None else self._check(gain, "gain", torch.float64, (nchan, nbin))
        seed, realization, bin0 = _noise_key(seed, realization, bin0)
        _lib.check(self.lib.efd_noise_fd(po, pg, nchan, nbin, bin0, seed, realization,
                                         int(bool(accumulate)), self._stream()),
                   "efd_noise_fd", self.lib)
        return out

    def noise_overlap_rows(self, rows, gain, seed, num_draws, real0=0, out=None):
        """out[r][p] = sum_c sum_k gain[c][k] Re(conj xi_{real0 + r}(c, k) rows[p][c][k]) for
        num_draws draws (efd_noise_overlap_rows: the noise is regenerated in registers, never
        written) as a float64 [num_draws][nrow] device tensor. rows: complex128
        [nrow][nchan][nbin] contiguous, nrow <= EFD_NOISE_MAX_ROWS; gain: float64 [nchan][nbin]
        or None (= 1). With gain = sqrt(4 df / S) an entry is <n_r | rows_p>. An entry does not
        depend on the other rows or draws, or on how the draws are split over calls."""
        torch = self.torch
        if rows.dim() != 3 or not 1 <= rows.shape[0] <= _lib.EFD_NOISE_MAX_ROWS:
            raise ValueError(f"rows: expected complex128 [1..{_lib.EFD_NOISE_MAX_ROWS}][nchan]"
                             f"[nbin], got {tuple(rows.shape)}")
        nrow, nchan, nbin = (int(v) for v in rows.shape)
        pr = self._check(rows, "rows", torch.complex128, (nrow, nchan, nbin))
        pg = None if gain is None else self._check(gain, "gain", torch.float64, (nchan, nbin))
        num_draws = int(num_draws)
        seed, real0, _ = _noise_key(seed, real0, 0)
        if num_draws < 0 or real0 + num_draws > 2 ** 32:
            raise ValueError("noise_overlap_rows: real0 + num_draws outside 0..2^32")
        if out is None:
            out = torch.empty((num_draws, nrow), dtype=torch.float64, device=self.device)
        po = self._check(out, "out", torch.float64, (num_draws, nrow))
        scr = self._scratch("_scr_nz", _lib.EFD_NOISE_SCRATCH)
        _lib.check(self.lib.efd_noise_overlap_rows(pr, nrow, pg, nchan, nbin, seed, real0,
                                                   num_draws, po, scr.data_ptr(),
                                                   self._stream()),
                   "efd_noise_overlap_rows", self.lib)
        return out

    def window_rows(self, h, windows, out):
        """out[j] = windows[j] * h for every window of one series (efd_window_rows): h
        complex128 [n]; windows: float64 [n] tensors, or None for the unwindowed copy; out:
        complex128 [len(windows)][>= n] with contiguous rows a fixed stride apart."""
        torch = self.torch
        n = int(h.numel())
        ph = self._check(h, "h", torch.complex128, (n,))
        nwin = len(windows)
        if not 1 <= nwin <= _lib.EFD_WINDOW_MAX_ROWS:
            raise ValueError(f"windows: expected 1..{_lib.EFD_WINDOW_MAX_ROWS}, got {nwin}")
        pout, stride, _, _ = self._rows(
            out, f"out: expected complex128 [{nwin}][>= {n}] on {self.device}", dim=2, nrow=nwin,
            nelem=n)
        ptrs = (ctypes.c_void_p * nwin)(*[
            None if x is None else self._check(x, "window", torch.float64, (n,))
            for x in windows])
        _lib.check(self.lib.efd_window_rows(ph, n, ptrs, nwin, pout, stride, self._stream()),
                   "efd_window_rows", self.lib)
        return out


def _noise_key(seed, realization, bin0):
    """(seed, realization, bin0) as the integers the C ABI takes: a 64-bit seed, a 32-bit
    realisation, a 64-bit first bin."""
    seed, realization, bin0 = int(seed), int(realization), int(bin0)
    if not 0 <= seed < 2 ** 64:
        raise ValueError("seed: an integer in 0..2^64 - 1")
    if not 0 <= realization < 2 ** 32:
        raise ValueError("realization: an integer in 0..2^32 - 1")
    if not 0 <= bin0 < 2 ** 64:
        raise ValueError("bin0: an integer in 0..2^64 - 1")
    return seed, realization, bin0
