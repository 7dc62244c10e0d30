"""Command line front end: ``python -m utmos_amd <command> [options]``.

Commands: ``select`` (the MI355X greedy selection, same flags and output as the reference's
``utmos select``, utmos/__main__.py:17-47 dispatches it the same way), ``convert`` (a VCF's genotypes -> the
reference's .jl part file, parsed on the GPU; utmos/convert.py) and ``version``.  ``select`` reads ``.vcf[.gz]``, ``.bcf``,
``.jl`` and ``.npz`` inputs directly.
"""
import sys

from . import __version__


def _usage():
    return (f"Utmos v{__version__} (MI355X build)\n"
            "usage: python -m utmos_amd COMMAND [OPTIONS]\n\n"
            "  select    pick the samples that capture the most variants (GPU); --samples-out / --represent-out: how much\n"
            "            of every sample's own variants each row captured\n"
            "  convert   VCF genotypes -> a .jl / .npz part file (GPU parser; BGZF inflated on the GPU)\n"
            "  overlap   count the variants every two samples share (GPU)\n"
            "  spectrum  carrier-count histogram of a sample list and its exact random-panel curve (GPU); --by-sample: every\n"
            "            sample's own singletons, doubletons, ...\n"
            "  filter    keep the variants that pass AF / carrier-count / list criteria and write them as a .utm store (GPU)\n"
            "  version   print the version and exit\n")


def _run_select(options):
    from .select import select_main
    select_main(options)
    return 0


def _run_version(_options):
    print(f"Utmos v{__version__}")
    return 0


def _run_convert(options):
    from .convert import cvt_main
    cvt_main(options)
    return 0


def _run_overlap(options):
    from .overlap import overlap_main
    overlap_main(options)
    return 0


def _run_spectrum(options):
    from .spectrum import spectrum_main
    spectrum_main(options)
    return 0


def _run_filter(options):
    from .variant_filter import filter_main
    filter_main(options)
    return 0


COMMANDS = {"filter": _run_filter, "select": _run_select, "version": _run_version, "convert": _run_convert, "overlap": _run_overlap,
            "spectrum": _run_spectrum}


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    if not argv or argv[0] in ("-h", "--help"):
        sys.stderr.write(_usage())
        return 0
    command, options = argv[0], argv[1:]
    if command not in COMMANDS:
        sys.stderr.write(f"unknown command {command!r}\n\n" + _usage())
        return 2
    return COMMANDS[command](options)


if __name__ == "__main__":
    sys.exit(main())
