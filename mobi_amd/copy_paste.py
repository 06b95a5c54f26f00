"""The copy-paste baseline of the test bench: `python -m mobi_amd.copy_paste <the arguments of python -m mobi_amd.bench_tree>` writes
the same result tree with the REFERENCE image pasted over each object instead of the sample -- the baseline row of the realism
table, which the reference's scripts/inference_test_bench.py makes with `--copy-paste` (scripts/inference_test_bench.py of this tree
hands a command line with that word to this command).

What differs from the plain command, as in the reference: the sampler runs ONE step whatever `--ddim_steps` says (the sample is
not shown, but the lidar side of the tree is that one-step sample), and the camera pictures come from the export launch in
copy-paste mode (`mobi_camera_copy_paste`, include/mobi_engine.h; `du.copy_paste_camera_patch` is its numpy form): the reference
resized onto the mask's box, the mask dilated 5 x 5 instead of blurred.  The loop is `bench_tree.run`; its lidar-on-camera overlays
are drawn on that frame.
`--dpm` is refused: the baseline is the reference's, whose command has no such sampler.
"""
from . import bench_tree


def parse(argv=None):
    """The test bench's parser (it has no flag for this) with `--no_overlays`; copy_paste set, one step forced."""
    opt = bench_tree.build_parser().parse_args(argv)
    if opt.dpm:
        raise SystemExit("python -m mobi_amd.copy_paste: --dpm is not offered (the baseline is the reference's: one DDIM or PLMS step)")
    opt.copy_paste = True
    opt.ddim_steps = 1
    return opt


def main(argv=None):
    bench_tree.run_command(parse(argv))


if __name__ == "__main__":
    main()
