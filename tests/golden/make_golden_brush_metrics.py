"""Golden vectors for the brush scores: what the REFERENCE returned on the cases of tests/brush_metrics_refs.py --
compute_lab_metrics and compute_lab_deltas (forger/metrics/color_metric.py:29-70), compute_transparency_metrics, the double
default_gaussian_smoothing and get_conservative_fg_bg (forger/metrics/geom_metric.py:126-162), the colour stream of
RandomState.random_tensor (forger/metrics/util.py:77-89) and lines of its metric files (to_file_line / ordered_dict_values,
forger/metrics/metric_main.py:48-72).  Only outputs are stored: the tests rebuild the inputs from the same seeds.  ``eps_ref`` is the
reference's own float32 distance from the float64 statement of brush_metrics_refs.py, the yardstick of the kernel's per-pixel bound.
Build container only.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_brush_metrics.py
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden_engine  # noqa: E402,F401  (puts the reference and its stubs for skimage / torchvision on the path)

tv = sys.modules["torchvision"]
tvt = types.ModuleType("torchvision.transforms")
tv.transforms = tvt
sys.modules.update({"torchvision.transforms": tvt, "lpips": types.ModuleType("lpips")})
import forger.metrics.color_metric as color_metric  # noqa: E402
import forger.metrics.geom_metric as geom_metric  # noqa: E402
import forger.metrics.util as metrics_util  # noqa: E402
import forger.metrics.metric_main as metric_main  # noqa: E402

import brush_metrics_refs as br  # noqa: E402


def main():
    out, eps = {}, 0.0
    for c in br.cases():
        name, n = c["name"], c["renders"].shape[0]
        k = c["geom_u8"].shape[0]
        geom = torch.from_numpy(br.geom_f32(c["geom_u8"]))
        g_n = geom[torch.arange(n) % k].unsqueeze(1)
        ren, tg = torch.from_numpy(c["renders"]), torch.from_numpy(c["targets"])
        lab = color_metric.compute_lab_metrics(tg, ren, g_n, lab_thresh=c["lab_thresh"], ignore_transparency=c["ignore"])
        deltas = color_metric.compute_lab_deltas(tg, ren, ignore_transparency=c["ignore"]).numpy()
        try:
            tr = geom_metric.compute_transparency_metrics(ren, g_n)
        except (RuntimeError, IndexError):                                  # torch.median of an empty selection
            alphas, blur = ren[:, 3], geom_metric.default_gaussian_smoothing(geom_metric.default_gaussian_smoothing(g_n)).squeeze(1)
            tr = {"BG_CLARITY_MEAN": 1 - torch.mean(alphas[blur > 0.999]).item(), "FG_OPACITY_MEDIAN": float("nan")}
        blur = geom_metric.default_gaussian_smoothing(geom_metric.default_gaussian_smoothing(geom.unsqueeze(1))).squeeze(1).numpy()
        fg, bg = geom_metric.get_conservative_fg_bg(geom.unsqueeze(1))
        out[f"{name}/scalars"] = np.array([tr["BG_CLARITY_MEAN"], tr["FG_OPACITY_MEDIAN"], lab["LAB_E%"], lab["LAB_L2"]], np.float64)
        out[f"{name}/deltas"] = deltas.astype(np.float32)
        out[f"{name}/blur"] = blur.astype(np.float32)
        out[f"{name}/conservative_fg"] = np.packbits(fg.numpy())
        out[f"{name}/conservative_bg"] = np.packbits(bg.numpy())
        eps = max(eps, float(np.abs(deltas.astype(np.float64) - br.deltas_f64(c["targets"], c["renders"], c["ignore"])).max()))
    out["eps_ref"] = np.float64(eps)
    state = metrics_util.RandomState(br.EVAL_SEED)
    out["color_stream"] = np.stack([state.random_tensor((5, 3)).numpy() for _ in range(4 * br.EVAL_ROUNDS)])
    keys = sorted(["LAB_E%", "LAB_L2", "BG_CLARITY_MEAN", "FG_OPACITY_MEDIAN"])
    sample = {"LAB_E%": 12.345678, "LAB_L2": 3.25, "BG_CLARITY_MEAN": 0.98765432, "FG_OPACITY_MEDIAN": 1.0}
    out["file_keys"] = np.array(keys)
    out["file_style_header"] = np.array("SEED            " + metric_main.to_file_line(keys))
    out["file_summary_header"] = np.array(metric_main.to_file_line(keys))
    out["file_sample_values"] = np.array([sample[k] for k in keys], np.float64)
    out["file_sample_style_line"] = np.array("{:<15}".format("594") + " " + metric_main.to_file_line(
        metric_main.ordered_dict_values(sample, keys), do_strip=False))
    path = os.path.join(HERE, "brush_metrics.npz")
    np.savez_compressed(path, **out)
    print("brush_metrics.npz:", len(out), "arrays, eps_ref", eps, os.path.getsize(path), "bytes")
    for c in br.cases():
        print(c["name"], out[f"{c['name']}/scalars"])


if __name__ == "__main__":
    main()
