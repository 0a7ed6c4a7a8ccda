"""``python -m peasoup_amd [peasoup flags]`` (or ``python -m peasoup_amd ffa
[ffaster flags]`` for the FFA search, ``python -m peasoup_amd sps [spsearch
flags]`` for the single-pulse search, ``python -m peasoup_amd cube [foldcube
flags]`` for the filterbank fold cubes of candidates, ``python -m peasoup_amd
burst [burstcube flags]`` for the cutouts of single-pulse candidates, ``python
-m peasoup_amd opt [cubeopt flags]`` for the DM / period / acceleration search
on fold cubes, ``python -m peasoup_amd bopt [burstopt flags]`` for the DM / width / time search on burst
cutouts, ``python -m peasoup_amd clean [rficlean flags]`` for the RFI excision, ``python -m peasoup_amd
scrunch [filscrunch flags]`` for the subbanded / time-scrunched filterbank, ``python -m peasoup_amd digi
[fildigi flags]`` for the 8-bit digitisation of a 16 / 32-bit or ascending-band filterbank, ``python -m peasoup_amd
fits [fits2fil flags]`` for the conversion of a search-mode PSRFITS file, ``python -m peasoup_amd inject
[filinject flags]`` for the injection of dispersed pulsars and bursts into a filterbank, ``python -m peasoup_amd jerk
[jerksearch flags]`` for the acceleration search repeated over jerk trials, ``python -m peasoup_amd orb
[orbsearch flags]`` for the one repeated over circular-orbit templates, ``python -m peasoup_amd sb
[sbsearch flags]`` for the sideband search for short orbits, ``python -m peasoup_amd oopt [orbopt flags]``
for the refinement of orbit candidates on a local template grid) -- the peasoup CLI as a
torchrun-compatible, one-process-per-GPU program:

    python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 \\
        -m peasoup_amd -i obs.fil --dm_end 1000 --acc_start -500 --acc_end 500 -n 3 --npdmp 128

Flags are identical to the native ``bin/peasoup`` (include/utils/cmdline.hpp).
A single process uses one GPU; the native CLI's ``-t`` thread-per-GPU mode
remains available in ``bin/peasoup``.

Failure handling: a failing rank prints its error with its
rank and exits immediately, so torchrun tears the group down instead of
letting the peers hang in a collective.  Elastic recovery is torchrun's
restart plus resume:

    python -m torch.distributed.run --max-restarts 3 ... -m peasoup_amd ... --checkpoint_dir ck/

re-runs the group after a failure and every rank skips the DM chunks whose
spill files (``ck/dm_<d0>_<d1>.psoc``) already exist.
"""
from __future__ import annotations

import sys


def _fail_hard(what: str, e: BaseException) -> None:
    """A failed rank must not leave its peers blocked in a collective: report
    with rank context and exit hard, which destroys this rank's RCCL
    communicator (the ncclCommAbort equivalent) and makes torchrun stop -- or,
    with --max-restarts, restart -- the worker group (a restart with
    --checkpoint_dir resumes from the per-DM spill files).  When a peer failed
    first (this rank's collective broke with it), the peer's record is
    reported instead of the broken connection."""
    import os
    import traceback

    from .parallel import dist as pdist

    rank = os.environ.get("RANK", "0")
    peer = pdist.peer_failure()
    if peer is not None:
        print(f"[rank {rank}] aborting: peer failure: {peer}", file=sys.stderr)
        sys.stderr.flush()
        if rank == "0":
            import time

            time.sleep(2.0)  # rank 0 hosts the store: let the other peers read the record
        os._exit(3)
    print(f"[rank {rank}] {what} failed: {e}", file=sys.stderr)
    pdist.report_failure(f"{type(e).__name__}: {e}")
    traceback.print_exc()
    sys.stderr.flush()
    sys.stdout.flush()
    os._exit(1)


def main(argv=None) -> int:
    from . import _C
    from .models.search import run_search
    from .parallel import dist as pdist

    argv = list(sys.argv if argv is None else argv)
    if len(argv) > 1 and argv[1] == "ffa":
        return _main_ffa(["ffaster"] + argv[2:])
    if len(argv) > 1 and argv[1] == "sps":
        return _main_sps(["spsearch"] + argv[2:])
    if len(argv) > 1 and argv[1] == "cube":
        return _main_cube(["foldcube"] + argv[2:])
    if len(argv) > 1 and argv[1] == "burst":
        return _main_burst(["burstcube"] + argv[2:])
    if len(argv) > 1 and argv[1] == "opt":
        return _main_opt(["cubeopt"] + argv[2:])
    if len(argv) > 1 and argv[1] == "bopt":
        return _main_bopt(["burstopt"] + argv[2:])
    if len(argv) > 1 and argv[1] == "clean":
        return _main_clean(["rficlean"] + argv[2:])
    if len(argv) > 1 and argv[1] == "scrunch":
        return _main_scrunch(["filscrunch"] + argv[2:])
    if len(argv) > 1 and argv[1] == "digi":
        return _main_digi(["fildigi"] + argv[2:])
    if len(argv) > 1 and argv[1] == "fits":
        return _main_fits(["fits2fil"] + argv[2:])
    if len(argv) > 1 and argv[1] == "inject":
        return _main_inject(["filinject"] + argv[2:])
    if len(argv) > 1 and argv[1] == "jerk":
        return _main_jerk(["jerksearch"] + argv[2:])
    if len(argv) > 1 and argv[1] == "orb":
        return _main_orbit(["orbsearch"] + argv[2:])
    if len(argv) > 1 and argv[1] == "sb":
        return _main_sb(["sbsearch"] + argv[2:])
    if len(argv) > 1 and argv[1] == "oopt":
        return _main_oopt(["orbopt"] + argv[2:])
    argv[0] = "peasoup"
    ok, exit_now, args = _C.parse_cmdline(argv)
    if not ok:
        print("Failed to parse command line arguments.", file=sys.stderr)
        return 1
    if exit_now:
        return 0
    if args.verbose:
        _C.set_log_level(2)
    try:
        res = run_search(args)
    except BaseException as e:  # noqa: BLE001 - any failure must tear the job down
        _fail_hard("peasoup", e)
    if res is not None and (args.verbose or args.progress_bar):
        print(f"Wrote {len(res.candidates)} candidates to {args.outdir}; "
              f"{res.performance['dm_accel_trials_per_sec']:.1f} DMxaccel trials/s over {int(res.performance['ranks'])} rank(s)")
    pdist.shutdown()
    return 0


def _main_ffa(argv) -> int:
    from . import _C
    from .models.ffa import run_ffa_search
    from .parallel import dist as pdist

    ok, exit_now, args = _C.parse_ffa_cmdline(argv)
    if not ok:
        print("Failed to parse command line arguments.", file=sys.stderr)
        return 1
    if exit_now:
        return 0
    try:
        res = run_ffa_search(args)
    except BaseException as e:  # noqa: BLE001 - same teardown policy as the search
        _fail_hard("ffa", e)
    if res is not None and args.verbose:
        print(f"Wrote {len(res.candidates)} FFA candidates to {args.outfilename}")
    pdist.shutdown()
    return 0


def _main_sps(argv) -> int:
    from . import _C
    from .models.singlepulse import run_single_pulse_search
    from .parallel import dist as pdist

    ok, exit_now, args = _C.parse_sp_cmdline(argv)
    if not ok:
        print("Failed to parse command line arguments.", file=sys.stderr)
        return 1
    if exit_now:
        return 0
    try:
        res = run_single_pulse_search(args)
    except BaseException as e:  # noqa: BLE001 - same teardown policy as the search
        _fail_hard("sps", e)
    if res is not None and args.verbose:
        print(f"Wrote {len(res.candidates)} single-pulse candidates to {args.outfilename}")
    pdist.shutdown()
    return 0


def _main_cube(argv) -> int:
    from . import _C
    from .models.foldcube import run_fold_cubes

    ok, exit_now, args = _C.parse_cube_cmdline(argv)
    if not ok:
        print("Failed to parse command line arguments.", file=sys.stderr)
        return 1
    if exit_now:
        return 0
    try:
        run = run_fold_cubes(args)
    except BaseException as e:  # noqa: BLE001 - same teardown policy as the search
        _fail_hard("cube", e)
    if run is not None and args.verbose:
        print(f"Wrote {run.ncand} fold cubes to {args.outfilename}")
    return 0


def _main_burst(argv) -> int:
    from . import _C
    from .models.burstcube import run_burst_cutouts

    ok, exit_now, args = _C.parse_burst_cmdline(argv)
    if not ok:
        print("Failed to parse command line arguments.", file=sys.stderr)
        return 1
    if exit_now:
        return 0
    try:
        run = run_burst_cutouts(args)
    except BaseException as e:  # noqa: BLE001 - same teardown policy as the search
        _fail_hard("burst", e)
    if run is not None and args.verbose:
        print(f"Wrote {run.ncand} burst cutouts to {args.outfilename}")
    return 0


def _main_opt(argv) -> int:
    from . import _C
    from .models.cubeopt import print_records, run_cube_opt

    ok, exit_now, args = _C.parse_opt_cmdline(argv)
    if not ok:
        print("Failed to parse command line arguments.", file=sys.stderr)
        return 1
    if exit_now:
        return 0
    try:
        run = run_cube_opt(args)
    except BaseException as e:  # noqa: BLE001 - same teardown policy as the search
        _fail_hard("opt", e)
    if run is not None and args.verbose:
        print_records(run)
        print(f"Wrote {run.ncand} cubeopt records to {args.outfilename}")
    return 0


def _main_bopt(argv) -> int:
    from . import _C
    from .models.burstopt import print_records, run_burst_opt

    ok, exit_now, args = _C.parse_bopt_cmdline(argv)
    if not ok:
        print("Failed to parse command line arguments.", file=sys.stderr)
        return 1
    if exit_now:
        return 0
    try:
        run = run_burst_opt(args)
    except BaseException as e:  # noqa: BLE001 - same teardown policy as the search
        _fail_hard("bopt", e)
    if run is not None and args.verbose:
        print_records(run)
        print(f"Wrote {run.ncand} burstopt records to {args.outfilename}")
    return 0


def _main_clean(argv) -> int:
    from . import _C
    from .models.rfi import clean_filterbank

    ok, exit_now, args = _C.parse_rfi_cmdline(argv)
    if not ok:
        print("Failed to parse command line arguments.", file=sys.stderr)
        return 1
    if exit_now:
        return 0
    try:
        mask = clean_filterbank(args)
    except BaseException as e:  # noqa: BLE001 - same teardown policy as the search
        _fail_hard("clean", e)
    if mask is not None and args.verbose:
        print(f"RFI excision: {mask.flagged_chans} of {mask.nchans} channels, {mask.flagged_blocks} of {mask.nblk} "
              f"blocks, {mask.flagged_cells} of {mask.nchans * mask.nblk} cells flagged")
    return 0


def _main_scrunch(argv) -> int:
    from . import _C
    from .models.scrunch import print_plan, scrunch_filterbank

    ok, exit_now, args = _C.parse_scrunch_cmdline(argv)
    if not ok:
        print("Failed to parse command line arguments.", file=sys.stderr)
        return 1
    if exit_now:
        return 0
    try:
        if args.plan:
            print_plan(args)
            return 0
        res = scrunch_filterbank(args)
    except BaseException as e:  # noqa: BLE001 - same teardown policy as the search
        _fail_hard("scrunch", e)
    if res is not None and args.verbose:
        print(f"filscrunch: {res['nout']} samples x {res['nsub']} subbands, mul {res['mul']}, sigma_ref "
              f"{res['sigma_ref']:g}, {res['nlive']} of {res['nsub']} subbands live")
        print("M: " + " ".join(str(int(m)) for m in res["M"]))
    return 0


def _main_digi(argv) -> int:
    from . import _C
    from .models.digi import digitise_filterbank

    ok, exit_now, args = _C.parse_digi_cmdline(argv)
    if not ok:
        print("Failed to parse command line arguments.", file=sys.stderr)
        return 1
    if exit_now:
        return 0
    try:
        res = digitise_filterbank(args)
    except BaseException as e:  # noqa: BLE001 - same teardown policy as the search
        _fail_hard("digi", e)
    if res is not None and args.verbose:
        print(f"fildigi: {res['nsamps']} samples x {res['nchans']} channels, nbad {int(res['nbad'].sum())}, nclip "
              f"{res['nclip']}, {res['nlive']} of {res['nchans']} channels live, gains {res['gain_min']:g} to "
              f"{res['gain_max']:g}")
    return 0


def _main_fits(argv) -> int:
    from . import _C
    from .models.psrfits import convert_psrfits

    ok, exit_now, args = _C.parse_fits_cmdline(argv)
    if not ok:
        print("Failed to parse command line arguments.", file=sys.stderr)
        return 1
    if exit_now:
        return 0
    try:
        res = convert_psrfits(args)
    except BaseException as e:  # noqa: BLE001 - same teardown policy as the search
        _fail_hard("fits", e)
    if res is not None and args.verbose:
        pols = "+".join(str(p) for p in res["pols"] if p >= 0)
        print(f"fits2fil: {res['rows']} rows, {res['ndropped']} dropped slots, polarisations {pols}, z {res['z']:g}, "
              f"{res['nsamps']} samples x {res['nchans']} channels, nbad {int(res['nbad'].sum())}, nclip "
              f"{res['nclip']}, {res['nlive']} of {res['nchans']} channels live, gains {res['gain_min']:g} to "
              f"{res['gain_max']:g}")
    return 0


def _main_inject(argv) -> int:
    from . import _C
    from .models.inject import inject_filterbank

    ok, exit_now, args = _C.parse_inject_cmdline(argv)
    if not ok:
        print("Failed to parse command line arguments.", file=sys.stderr)
        return 1
    if exit_now:
        return 0
    try:
        res = inject_filterbank(args)
    except BaseException as e:  # noqa: BLE001 - same teardown policy as the search
        _fail_hard("inject", e)
    if res is not None and args.verbose:
        print(f"filinject: {res['nsamps']} samples x {res['nchans']} channels, {res['nsig']} signals, nclip "
              f"{res['nclip']}, {res['nlive']} of {res['nchans']} channels live, {res['chunks']} chunk(s)")
        for i, (s, t) in enumerate(zip(res["signals"], res["truth"])):
            print(f"  signal {i} ({s.kind}): {int(res['touched'][i])} samples touched, {t[0]} pulses, peak {t[1]:g} "
                  f"levels, expected S/N {t[2]:g}")
    return 0


def _main_jerk(argv) -> int:
    from . import _C
    from .models.jerk import run_jerk_search

    ok, exit_now, args = _C.parse_jerk_cmdline(argv)
    if not ok:
        print("Failed to parse command line arguments.", file=sys.stderr)
        return 1
    if exit_now:
        return 0
    try:
        res = run_jerk_search(args)
    except BaseException as e:  # noqa: BLE001 - same teardown policy as the search
        _fail_hard("jerk", e)
    if res is not None and args.search.verbose:
        print(f"jerksearch: {len(res.candidates)} candidates from {res.jerk_trials} DM-jerk trials "
              f"({res.accel_trials} acceleration trials) to {args.outfilename}")
    return 0


def _main_orbit(argv) -> int:
    from . import _C
    from .models.orbit import run_orbit_search

    ok, exit_now, args = _C.parse_orbit_cmdline(argv)
    if not ok:
        print("Failed to parse command line arguments.", file=sys.stderr)
        return 1
    if exit_now:
        return 0
    try:
        res = run_orbit_search(args)
    except BaseException as e:  # noqa: BLE001 - same teardown policy as the search
        _fail_hard("orb", e)
    if res is not None and args.search.verbose:
        print(f"orbsearch: {len(res.candidates)} candidates from {res.template_trials} DM-template trials "
              f"({res.accel_trials} acceleration trials) to {args.outfilename}")
    return 0


def _main_oopt(argv) -> int:
    from . import _C
    from .models.orbopt import print_records, run_orbit_optimise

    ok, exit_now, args = _C.parse_oopt_cmdline(argv)
    if not ok:
        print("Failed to parse command line arguments.", file=sys.stderr)
        return 1
    if exit_now:
        return 0
    try:
        res = run_orbit_optimise(args)
    except BaseException as e:  # noqa: BLE001 - same teardown policy as the search
        _fail_hard("oopt", e)
    if res is not None and args.verbose:
        print_records(res)
        print(f"orbopt: {len(res.records)} candidates to {args.outfilename}")
    return 0


def _main_sb(argv) -> int:
    from . import _C
    from .models.sideband import run_sideband_search

    ok, exit_now, args = _C.parse_sb_cmdline(argv)
    if not ok:
        print("Failed to parse command line arguments.", file=sys.stderr)
        return 1
    if exit_now:
        return 0
    try:
        res = run_sideband_search(args)
    except BaseException as e:  # noqa: BLE001 - same teardown policy as the search
        _fail_hard("sb", e)
    if res is not None and args.search.verbose:
        print(f"sbsearch: {len(res.candidates)} candidates from {res.events} events of "
              f"{len(res.setup.dm_list)} DM trials to {args.outfilename}")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
