"""DAVIS J&F of a results directory against its annotations (the `compute_metrics` step of inference/run_experiments.py):

    python -m xmem2_amd.evaluate --gt /data/DAVIS/Annotations/480p --pred /results [--csv scores.csv]

`--pred` is laid out as the launcher writes it, `<pred>/<video>/masks/*.png`; `--gt` holds `<gt>/<video>/*.png`.  A video whose
`masks/` is absent or empty but which has `<pred>/<video>/tracks.json` (config['save_tracks']) is scored from the tracks, decoded on
the device (`--pred-format` forces one source).  Prints per-video J, F and J&F and the dataset means (the mean over videos of the
per-video means).
"""
import argparse
import sys


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description='DAVIS J (region similarity) and F (boundary accuracy) of predicted masks.')
    ap.add_argument('--gt', required=True, help='annotation directory: <gt>/<video>/*.png')
    ap.add_argument('--pred', required=True, help='results directory: <pred>/<video>/masks/*.png (the launcher\'s --out)')
    ap.add_argument('--csv', default=None, help='also write the per-video table here')
    ap.add_argument('--workers', type=int, default=8, help='host threads decoding PNGs')
    ap.add_argument('--pred-format', default='auto', choices=('auto', 'png', 'tracks'),
                    help='what is read per video under --pred: png = masks/*.png; tracks = tracks.json, decoded and scored on the '
                         'device; auto (default) = the PNGs where masks/ holds a file, else tracks.json where it exists')
    return ap.parse_args(argv)


def main(argv=None):
    args = parse_args(argv)
    from .metrics import compute_metrics
    df = compute_metrics(args.gt, args.pred, workers=args.workers, pred_format=args.pred_format)
    width = max(10, max(len(str(n)) for n in df.index))
    print(f'{"video":<{width}}  {"J":>8}  {"F":>8}  {"J&F":>8}')
    for name, row in df.iterrows():
        print(f'{str(name):<{width}}  {row["iou"]:8.4f}  {row["f"]:8.4f}  {row["jf"]:8.4f}')
    print(f'{"mean":<{width}}  {df["iou"].mean():8.4f}  {df["f"].mean():8.4f}  {df["jf"].mean():8.4f}  ({len(df)} videos)')
    if args.csv:
        df.to_csv(args.csv)
    return 0


if __name__ == '__main__':
    sys.exit(main())
