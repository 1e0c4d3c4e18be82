"""Test helper: the store rules of the row-map launchers (include/orcai_hip.h) in Python, on rows that are any Python values."""


def _families_store(dst, written, img, w, b, r0, fams):
    """The store rule of orcai_pool_res_add_scatter_families for image b of window w (source rows from r0 = b's recording row)."""
    for r in range(len(img)):
        rr = r0 + r
        if not ((r >= w.r_lo or rr == r) and r < w.r_hi):
            continue
        for f in fams:
            rel = rr - f.offset - f.keep_lo
            if rel < 0:
                continue
            assert f.keep_hi - f.keep_lo <= 2 * f.period  # what the launcher checks: the kernel visits two images per family
            for j in (rel // f.period, rel // f.period - 1):
                y = rr - f.offset - j * f.period
                if 0 <= j < f.count and y < f.keep_hi:
                    dst[f.planes][f.image + j][y] = img[r]
                    written[f.planes][f.image + j, y] += 1


def _scatter_store(dst, written, img, w, r0, rows, period, nsnip):
    """The store rule of orcai_pool_res_add_scatter (one family: the snippets)."""
    for r in range(len(img)):
        rr = r0 + r
        if not ((r >= w.r_lo or rr == r) and r < w.r_hi):
            continue
        for sn in (rr // period, rr // period - 1):
            y = rr - sn * period
            if 0 <= sn < nsnip and w.keep_lo <= y < w.keep_hi:
                dst[sn][y] = img[r]
                written[sn, y] += 1
