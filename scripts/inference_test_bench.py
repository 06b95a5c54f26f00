import os, sys; sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))   # noqa: E401,E702
# the reference's drivers call this path: python3 scripts/inference_test_bench.py ... [--copy-paste]
if "--copy-paste" in sys.argv[1:]:                          # the baseline row is a command of its own: the word goes, the rest stays
    from mobi_amd.copy_paste import main
    main([a for a in sys.argv[1:] if a != "--copy-paste"])
else:                                                       # the test bench with the reference's whole tree, overlays included
    from mobi_amd.bench_tree import main
    main()
