"""The image-source kernels' own times from rocprofv3 kernel traces ("Image sources"): for every *_kernel_trace.csv given,
the dispatches of hare_image_mirror, hare_image_pairs, hare_image_deposit[_dir], the direct sound's kernels and the flags-only occlusion
kernels, grouped by kernel and grid (the grid tells the K = 8 call from the map's, and the image sources' occlusion launch of
2 * "image_max_pairs" slots from the direct sound's of K), with count, median, min and max in microseconds.  The traces come from
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/receiver_rate.py hall --source --direct --image --image-cull N
one run per N.  Prints ONE JSON line.  usage: python tools/image_kernel_times.py LABEL=trace.csv [LABEL=trace.csv ..]"""
import csv
import json
import statistics
import sys

WANTED = ("hare_image", "hare_direct_", "_occl")


def summarise(path):
    groups = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            name = row["Kernel_Name"].split("(")[0]
            if not any(w in name for w in WANTED):
                continue
            grid = "x".join(str(int(row[k])) for k in ("Grid_Size_X", "Grid_Size_Y") if k in row)
            groups.setdefault((name, grid), []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
    return [{"kernel": k, "grid": g, "calls": len(v), "median_us": round(statistics.median(v), 2), "min_us": round(min(v), 2),
             "max_us": round(max(v), 2)} for (k, g), v in sorted(groups.items())]


if __name__ == "__main__":
    if len(sys.argv) < 2 or any("=" not in a for a in sys.argv[1:]):
        sys.exit(__doc__)
    print(json.dumps({a.split("=", 1)[0]: summarise(a.split("=", 1)[1]) for a in sys.argv[1:]}))
