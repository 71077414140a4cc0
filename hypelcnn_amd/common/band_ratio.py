"""Per-band ratio statistics of the shadow GANs and their figure (reference gan_common.py print_stats :210-219 and
plot_overall_info :395-414, utilities/measure_targets_shadow_ratio.py).

    ratio = num / den * scale          float32, where the spectra are (hypel_band_ratio_f32)
    kept  = rows of ratio that are finite in every band
    pQ    = numpy.percentile(ratio[kept].astype(float64), Q, axis=0)

The order statistics come from one hypel_column_rank_select_f32 launch for all ranks the percentiles interpolate
between; only those [n_ranks, bands] values, the count and the two moment vectors leave the device.  The interpolation
is NumPy's linear rule evaluated in float64 (device_scene.percentile_from_ranks): the result equals numpy.percentile of
the float64 ratios bit for bit.  The reference interpolates float32 ratios in float32, a rule that depends on the NumPy
version and differs from this one by about one float32 ulp -- invisible in the figure, and the only deviation."""
import json
import os

import numpy
import torch

from hypelcnn_amd.backend import COLUMN_RANK_MAX_BANDS, COLUMN_RANK_MAX_RANKS, COLUMN_RANK_WS_WORDS, Ref
from hypelcnn_amd.common.device_scene import percentile_from_ranks, percentile_ranks


def _rows(backend, a):
    """-> (Ref, row stride, n, bands) of a [n, bands] float32 matrix on the backend's device.  A tensor whose band
    axis is contiguous is read where it is, whatever its row stride; anything else is copied (NumPy arrays: uploaded)."""
    if not torch.is_tensor(a):
        a = numpy.asarray(a, numpy.float32)
        a = backend.upload(a.reshape(a.shape[0], -1)).view(a.shape[0], -1)
    if a.dim() != 2:
        a = a.reshape(a.shape[0], -1)
    if a.dtype != torch.float32 or (a.shape[1] > 1 and a.stride(1) != 1) or (a.shape[0] > 1 and a.stride(0) < a.shape[1]):
        a = a.to(torch.float32).contiguous()
    n, bands = int(a.shape[0]), int(a.shape[1])
    ld = int(a.stride(0)) if n > 1 else bands
    flat = a.as_strided(((n - 1) * ld + bands,), (1,))
    return Ref(flat), ld, n, bands


def percentile_key(q):
    return f"p{q:g}"


def band_ratio_stats(backend, num, den, scale, percentiles=(10, 50, 90)):
    """Statistics of num / den * scale over the rows that are finite in every band.  num, den: [n, bands] float32
    device tensors (row-strided views are read in place) or NumPy arrays; scale: [bands] or None.  -> dict with
    `samples`, `kept`, one `p<q>` per percentile, `mean` and `std` (population), float64 [bands] arrays -- NaN when no
    row is kept."""
    num_ref, ld_num, n, bands = _rows(backend, num)
    den_ref, ld_den, n_den, bands_den = _rows(backend, den)
    if (n, bands) != (n_den, bands_den) or n < 1 or bands < 1:
        raise ValueError(f"band_ratio_stats: numerator [{n}, {bands}] and denominator [{n_den}, {bands_den}] must be "
                         f"equal, non-empty shapes")
    scale_ref = None
    if scale is not None:
        s = scale if torch.is_tensor(scale) else backend.upload(numpy.asarray(scale, numpy.float32))
        s = s.to(torch.float32).reshape(-1).contiguous()
        if s.numel() != bands:
            raise ValueError(f"band_ratio_stats: {s.numel()} scales for {bands} bands")
        scale_ref = Ref(s)
    ratio = backend.empty(n * bands)
    row_ok = backend.empty(n, torch.uint8)
    count = backend.empty(1, torch.int64)
    backend.call("band_ratio_f32", num_ref, ld_num, den_ref, ld_den, n, bands, scale_ref, Ref(ratio), bands, Ref(row_ok),
                 Ref(count))
    kept = int(count.cpu()[0])
    out = {"samples": n, "kept": kept}
    nan = numpy.full(bands, numpy.nan)
    if kept == 0:
        out.update({percentile_key(q): nan.copy() for q in percentiles}, mean=nan.copy(), std=nan.copy())
        return out
    plan = [percentile_ranks(kept, q) for q in percentiles]
    ranks = sorted({r for lo, hi, _ in plan for r in (lo, hi)})
    values = {}
    ws = backend.empty(min(bands, COLUMN_RANK_MAX_BANDS) * COLUMN_RANK_WS_WORDS, torch.int32)
    for at in range(0, len(ranks), COLUMN_RANK_MAX_RANKS):
        part = ranks[at:at + COLUMN_RANK_MAX_RANKS]
        host_ranks = torch.tensor(part, dtype=torch.int64)  # read by the call itself, before anything is launched
        got = numpy.empty((len(part), bands), numpy.float64)
        for b0 in range(0, bands, COLUMN_RANK_MAX_BANDS):  # (one window for any real spectrum)
            width = min(COLUMN_RANK_MAX_BANDS, bands - b0)
            picked = backend.empty(len(part) * width)
            backend.call("column_rank_select_f32", Ref(ratio, b0), bands, n, width, Ref(row_ok), kept, Ref(host_ranks),
                         len(part), Ref(picked), Ref(ws))
            got[:, b0:b0 + width] = picked.cpu().numpy().reshape(len(part), width)
        values.update(zip(part, got))
    for q, (lo, hi, t) in zip(percentiles, plan):
        out[percentile_key(q)] = percentile_from_ranks(values[lo], values[hi], t, numpy.float64)
    out["mean"], out["std"] = _moments(ratio.view(n, bands), row_ok.bool(), kept)
    return out


def _moments(ratio, keep, kept, chunk_elements=1 << 22):
    """create_stats' moments over the kept rows -- float64 mean and population std, two passes -- taken a block of rows
    at a time, so that the float64 copy is 32 MiB at the most and not 8 bytes per element of a whole scene's pairs."""
    n, bands = ratio.shape
    step = max(1, chunk_elements // bands)
    total = torch.zeros(bands, dtype=torch.float64, device=ratio.device)
    for r0 in range(0, n, step):
        total += ratio[r0:r0 + step][keep[r0:r0 + step]].double().sum(0)
    mean = total / kept
    squares = torch.zeros_like(total)
    for r0 in range(0, n, step):
        d = ratio[r0:r0 + step][keep[r0:r0 + step]].double() - mean
        squares += (d * d).sum(0)
    return mean.cpu().numpy(), torch.sqrt(squares / kept).cpu().numpy()


def plot_band_ratio(bands, mean, lower, upper, iteration, plt_name, log_dir):
    """The reference's band-ratio figure: the centre as points joined by a line over the band wavelengths, the band
    between `lower` and `upper` shaded, ratio axis fixed to [-1, 4]; written to <log_dir>/<plt_name>_<iteration>.pdf.
    Drawn on a Figure of its own: no pyplot, no global state.  -> the path, or None without matplotlib."""
    try:
        from matplotlib.figure import Figure
    except ImportError:
        print("matplotlib is not installed: the band-ratio figure is not drawn (its numbers are in the .json)")
        return None
    fig = Figure()
    ax = fig.add_subplot(1, 1, 1)
    ax.scatter(bands, mean, s=10)
    ax.plot(bands, mean)
    ax.fill_between(bands, lower, upper, alpha=0.2)
    ax.set_xlabel("Spectral band(nm)", fontsize=14)
    ax.set_ylabel("Ratio between generated and original samples", fontsize=14)
    ax.set_ylim([-1, 4])
    ax.set_yticks(list(range(-1, 5)))
    ax.tick_params(labelsize=14)
    ax.grid(True)
    path = os.path.join(log_dir, f"{plt_name}_{iteration}.pdf")
    fig.savefig(path, format="pdf", dpi=300, bbox_inches="tight")
    return path


def _listed(v):
    return [float(x) if numpy.isfinite(x) else None for x in numpy.asarray(v, numpy.float64).reshape(-1)]


def write_band_ratio(log_dir, plt_name, iteration, bands, stats, centre, lower=None, upper=None):
    """<plt_name>_<iteration>.json with the numbers (always) and .pdf with the figure (when a row was kept and
    matplotlib imports).  centre / lower / upper: keys of `stats`, or arrays.  -> the record written."""
    record = {"step": int(iteration), "bands": _listed(bands), "samples": int(stats["samples"]),
              "kept": int(stats["kept"])}
    for key, value in stats.items():
        if key not in record:
            record[key] = _listed(value)
    os.makedirs(log_dir, exist_ok=True)
    with open(os.path.join(log_dir, f"{plt_name}_{int(iteration)}.json"), "w") as f:
        json.dump(record, f)
    if stats["kept"] > 0:
        pick = [stats[v] if isinstance(v, str) else v for v in (centre, lower, upper)]
        plot_band_ratio(numpy.asarray(bands, numpy.float64), *pick, int(iteration), plt_name, log_dir)
    return record
