"""The settings of the configurations the reference trains, configs/Final_test/*.yaml (build container only).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_final_configs.py <reference checkout>

Every file is read with yaml.safe_load; nothing else of the reference is kept.  Dropped per file: every path (keys ending in
_path), every list or folder of data (data_list_*, data_folder_*, seg_list_*), the logging cadences (LOGGING) and the FID
keys (any key with "fid" in it, inception_moment_path).  `display_size` stays: the trainer's constructor reads it.

Output: tests/golden/golden_final_configs.json -- {file name without .yaml: settings}, keys sorted."""
import glob
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "golden_final_configs.json")
LOGGING = ("image_save_iter", "image_display_iter", "snapshot_save_iter", "log_iter")


def dropped(key):
    return (key.endswith("_path") or key.startswith(("data_list_", "data_folder_", "seg_list_")) or key in LOGGING
            or "fid" in key)


def settings(cfg):
    out = {k: v for k, v in cfg.items() if not dropped(k)}
    for k, v in out.items():
        assert isinstance(v, (int, float, str, dict)) and not isinstance(v, bool), (k, v)
        assert not (isinstance(v, str) and ("/" in v or v.endswith((".txt", ".pth", ".npz")))), (k, v)
    return out


def main(ref):
    import yaml
    files = sorted(glob.glob(os.path.join(ref, "configs", "Final_test", "*.yaml")))
    assert files, "no configs/Final_test/*.yaml under %s" % ref
    out = {}
    for f in files:
        with open(f) as fh:
            out[os.path.splitext(os.path.basename(f))[0]] = settings(yaml.safe_load(fh))
    with open(OUT, "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("wrote %s: %s" % (OUT, ", ".join(out)))


if __name__ == "__main__":
    main(sys.argv[1])
