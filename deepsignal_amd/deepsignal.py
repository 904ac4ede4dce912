"""`deepsignal call_mods` command line — the reference's flag surface for this sub-command
(reference deepsignal/deepsignal.py:236-326, defaults included), driving the MI355X engine — plus `extract`, the
host-side step that produces call_mods' feature-TSV input (deepsignal.py:155-234), and `call_freq`, the per-site frequency table
from call_mods' result files (scripts/call_modification_frequency.py), and `combine_strands`, both strands of each CpG of that
table combined (scripts/combine_two_strands_frequency.py).

Multi-GPU: one process per GPU, e.g.
    python -m torch.distributed.run --nnodes=1 --nproc-per-node 8 --master-addr 127.0.0.1 \
        -m deepsignal_amd.deepsignal call_mods -i features.tsv -m model.ckpt -o calls.tsv
reads are dealt to the ranks, rank 0 gathers the results over RCCL and writes the file."""
from __future__ import absolute_import

import argparse
import sys

from .utils.process_utils import display_args, str2bool


def main_call_mods(args):
    from .call_modifications import call_mods
    display_args(args)
    # the reference's tuple, in the reference's order (deepsignal.py:83-84); methy_label is fixed to 1 there (:78-79)
    f5_args = (str2bool(args.recursively), args.corrected_group, args.basecall_subgroup, args.reference_path,
               str2bool(args.is_dna), args.normalize_method, args.motifs, args.mod_loc, 1, args.f5_batch_num,
               args.positions)
    call_mods(args.input_path, args.model_path, args.result_file, args.kmer_len, args.cent_signals_len,
              args.batch_size, args.learning_rate, args.class_num, args.nproc, str2bool(args.is_gpu),
              str2bool(args.is_rnn), str2bool(args.is_base), str2bool(args.is_cnn), f5_args,
              precision=args.precision, engine_batch=args.engine_batch, extract_on=args.extract_on,
              recheck_margin=args.recheck_margin, recheck_precision=args.recheck_precision, parse_on=args.parse_on,
              freq_file=args.freq_file, freq_bed=args.freq_bed, freq_sort=args.freq_sort, freq_prob_cf=args.freq_prob_cf,
              freq_device=args.freq_device)


def main_extraction(args):
    from .extract_features import extract_features
    display_args(args)
    extract_features(args.fast5_dir, str2bool(args.recursively), args.reference_path, str2bool(args.is_dna),
                     args.f5_batch_num, args.write_path, args.nproc, args.corrected_group, args.basecall_subgroup,
                     args.normalize_method, args.motifs, args.mod_loc, args.kmer_len, args.cent_signals_len,
                     args.methy_label, args.positions, str2bool(args.w_is_dir), args.w_batch_num,
                     extract_on=args.extract_on, device=args.device, engine_batch=args.engine_batch)


def main_call_freq(args):
    from .call_modification_frequency import main as freq_main
    argv = []
    for path in args.input_path:
        argv += ["-i", path]
    argv += ["-o", args.result_file, "--prob_cf", repr(args.prob_cf), "--on", args.on]
    argv += ["--bed"] if args.bed else []
    argv += ["--sort"] if args.sort else []
    argv += ["--file_uid", args.file_uid] if args.file_uid is not None else []
    argv += ["--device", str(args.device)] if args.device is not None else []
    argv += ["--combine_ref", args.combine_ref] if args.combine_ref is not None else []
    argv += ["--combine_contig", args.combine_contig] if args.combine_contig is not None else []
    return freq_main(argv)


def main_combine_strands(args):
    from .combine_strands import combine_strands
    combine_strands(args.frequency_fp, args.ref_fp, args.contig, args.result_file, args.on, args.device or 0)
    return 0


def main_evaluate(args):
    from .evaluate_mods_call import run
    return run(args)


def main_denoise(args):
    from .denoise import run
    return run(args)


def main_train(args):
    from .train_model import run
    return run(args)


def _names_freq_file(argv) -> bool:
    """Does the command line give call_mods' --freq_file (spelled out, abbreviated as argparse allows, or with '=')?"""
    for a in argv:
        name = a.split("=", 1)[0]
        if len(name) >= len("--freq_f") and "--freq_file".startswith(name):
            return True
    return False


def build_parser(freq_file_given=True):
    """freq_file_given: call_mods' --result_file is required unless --freq_file is on the command line; main() passes what it sees
    there, so that without --freq_file argparse raises the error it always raised, with every missing flag in it."""
    parser = argparse.ArgumentParser(prog="deepsignal", description="call_mods on MI355X (gfx950)")
    sub = parser.add_subparsers(title="modules", dest="module")
    # `extract`: the step before the path -- fast5 -> feature TSV (reference deepsignal/deepsignal.py:155-234, same flags)
    e = sub.add_parser("extract", description="extract features from fast5 files (on the host, or with --extract_on gpu the numeric part and the row text on the GPU; HDF5 through h5py, or deepsignal_amd.minihdf5 where h5py is absent)")
    g = e.add_argument_group("INPUT")
    g.add_argument("--fast5_dir", "-i", required=True)
    g.add_argument("--recursively", "-r", default="yes")
    g.add_argument("--corrected_group", default="RawGenomeCorrected_000")
    g.add_argument("--basecall_subgroup", default="BaseCalled_template")
    g.add_argument("--is_dna", default="yes")
    g.add_argument("--reference_path", default=None)
    g = e.add_argument_group("EXTRACTION")
    g.add_argument("--normalize_method", default="mad", choices=["mad", "zscore"])
    g.add_argument("--methy_label", type=int, default=1, choices=[1, 0])
    g.add_argument("--kmer_len", type=int, default=17)
    g.add_argument("--cent_signals_len", type=int, default=360)
    g.add_argument("--motifs", default="CG")
    g.add_argument("--mod_loc", type=int, default=0)
    g.add_argument("--positions", default=None)
    g = e.add_argument_group("OUTPUT")
    g.add_argument("--write_path", "-o", required=True)
    g.add_argument("--w_is_dir", default="no")
    g.add_argument("--w_batch_num", type=int, default=200)
    e.add_argument("--nproc", "-p", type=int, default=1)
    e.add_argument("--f5_batch_num", type=int, default=50)
    g = e.add_argument_group("ENGINE")
    g.add_argument("--extract_on", default="cpu", choices=["cpu", "gpu"],
                   help="gpu: normalisation, per-site features and the rows' text are computed on the GPU (no model needed); the "
                        "workers only read the fast5 files. Rows equal the cpu route's, except the signals of a site whose middle "
                        "base alone has >= cent_signals_len samples (an ordered subsample on both routes)")
    g.add_argument("--device", type=int, default=0, help="GPU ordinal of --extract_on gpu")
    g.add_argument("--engine_batch", type=int, default=4096, help="most sites per device pass of --extract_on gpu")
    e.set_defaults(func=main_extraction)
    p = sub.add_parser("call_mods", description="call modifications")
    g = p.add_argument_group("INPUT")
    g.add_argument("--input_path", "-i", required=True,
                   help="a file of extracted features (fast5 dirs need `extract` first)")
    g.add_argument("--f5_batch_num", type=int, default=50)
    g = p.add_argument_group("CALL")
    g.add_argument("--model_path", "-m", required=True,
                   help="TensorFlow checkpoint prefix of a reference-trained model (<prefix>.index + .data-*), "
                        "or a DSAMDW01 weight file")
    g.add_argument("--precision", default="fp32", choices=["fp32", "bf16x3", "fp16x2", "bf16", "bf16_all"],
                   help="fp32 (reference numerics, native fp32 matrix instructions); bf16x3 (fp32-class results: fp32 operands carried "
                        "as three bf16 terms on the bf16 matrix pipe, held to the fp32 parity bars); fp16x2 (fp32-class results on two fp16 "
                        "terms and three products per MAC, held to the same bars; matrix operands -- folded weights and the activations "
                        "of conv_layer2 onwards -- must stay within +-65504, a site beyond that comes out NaN); bf16 / bf16_all (bf16 conv+FC "
                        "operands with fp32 accumulate: fast, probabilities good to ~1e-2 only)")
    g.add_argument("--recheck_margin", type=float, default=0.0,
                   help="cascaded precision, with --precision bf16 / bf16_all: sites whose |prob_1 - prob_0| comes out below this "
                        "margin are run again in --recheck_precision and take that result (default 0 = off; an fp32-class "
                        "--precision has nothing to recheck and is refused)")
    g.add_argument("--recheck_precision", default="fp32", choices=["fp32", "bf16x3", "fp16x2"],
                   help="the mode of the second forward of --recheck_margin")
    g.add_argument("--extract_on", default="cpu", choices=["cpu", "gpu"],
                   help="fast5-directory input only: compute the per-site features on the host (cpu, default) or on the GPU next "
                        "to the forward (gpu; same features bit for bit, except that a middle base of >= cent_signals_len samples "
                        "is subsampled by a seeded hash instead of Python's unseeded random)")
    g.add_argument("--parse_on", default="cpu", choices=["cpu", "gpu"],
                   help="feature-file input only: parse the rows' numbers on the host threads (cpu, default) or on the GPU straight "
                        "into the forward's inputs (gpu; the host only finds the rows). Same output bytes: rows in a form the device "
                        "does not parse go through the host parser")
    g.add_argument("--engine_batch", type=int, default=0,
                   help="sites per GPU forward the engine is created for (default 0: the larger of --batch_size and 4096; results do "
                        "not depend on it, device and pinned memory grow with it -- lower it on a small or shared GPU; the "
                        "environment variable DS_ENGINE_BATCH does the same)")
    g.add_argument("--is_cnn", default="yes")
    g.add_argument("--is_rnn", default="yes")
    g.add_argument("--is_base", default="yes")
    g.add_argument("--kmer_len", "-x", type=int, default=17)
    g.add_argument("--cent_signals_len", "-y", type=int, default=360)
    g.add_argument("--batch_size", "-b", type=int, default=512,
                   help="the reference's rows per sess.run; here the granularity rows are handed to the engine in, NOT the sites per "
                        "GPU forward (see --engine_batch): a site's result does not depend on its batch mates")
    g.add_argument("--learning_rate", "-l", type=float, default=0.001)
    g.add_argument("--class_num", "-c", type=int, default=2)
    g = p.add_argument_group("OUTPUT")
    g.add_argument("--result_file", "-o", required=not freq_file_given, default=None,
                   help="the calls, one row per (read, site); may be left out only with --freq_file")
    g.add_argument("--freq_file", default=None,
                   help="also write the per-site frequency table `call_freq` computes from the result file, straight from the forward's "
                        "results (no result text is parsed; without --result_file none is written); same bytes as call_freq on the "
                        "result file. Single process only")
    g.add_argument("--freq_bed", action="store_true", default=False, help="--freq_file: bedMethyl (call_freq --bed)")
    g.add_argument("--freq_sort", action="store_true", default=False, help="--freq_file: sites sorted by (chromosome, position) (call_freq --sort)")
    g.add_argument("--freq_prob_cf", type=float, default=0.0, help="--freq_file: leave out calls with |prob_0 - prob_1| below this (call_freq --prob_cf)")
    g.add_argument("--freq_device", type=int, default=None, help="--freq_file: GPU ordinal of the aggregation (default: the forward's)")
    g = p.add_argument_group("EXTRACTION")
    g.add_argument("--recursively", "-r", default="yes")
    g.add_argument("--corrected_group", default="RawGenomeCorrected_000")
    g.add_argument("--basecall_subgroup", default="BaseCalled_template")
    g.add_argument("--is_dna", default="yes")
    g.add_argument("--normalize_method", default="mad", choices=["mad", "zscore"])
    g.add_argument("--motifs", default="CG")
    g.add_argument("--mod_loc", type=int, default=0)
    g.add_argument("--positions", default=None)
    g.add_argument("--reference_path", default=None)
    p.add_argument("--nproc", "-p", type=int, default=1)
    p.add_argument("--is_gpu", default="no", choices=["yes", "no"])
    p.set_defaults(func=main_call_mods)
    parser.call_mods_parser = p      # main() raises the usage errors that span several flags
    # `call_freq`: the step after the path -- call_mods result files -> per-site frequency table or bedMethyl (the reference's later
    # releases expose scripts/call_modification_frequency.py under this name; same flags, plus --on / --device)
    f = sub.add_parser("call_freq", description="calculate the modification frequency of every site from call_mods result files")
    f.add_argument("--input_path", "-i", action="append", type=str, required=True,
                   help="a result file of call_mods (may be .gz) or a directory of them; may be given more than once")
    f.add_argument("--result_file", "-o", type=str, required=True)
    f.add_argument("--bed", action="store_true", default=False, help="write bedMethyl instead of the 11-column table")
    f.add_argument("--sort", action="store_true", default=False, help="sort the sites by (chromosome, position)")
    f.add_argument("--prob_cf", type=float, default=0.0, help="leave out calls with |prob_0 - prob_1| below this")
    f.add_argument("--file_uid", type=str, default=None, help="with a directory: only the files whose name holds this")
    f.add_argument("--on", default="cpu", choices=["cpu", "gpu"],
                   help="gpu: rows parsed and aggregated on the GPU (the host only finds them); same output bytes")
    f.add_argument("--device", type=int, default=None, help="GPU ordinal of --on gpu (default 0)")
    f.add_argument("--combine_ref", type=str, default=None,
                   help="a genome reference (FASTA): also write the table with both strands of each CpG combined "
                        "(`combine_strands` on the result file; honours --on / --device)")
    f.add_argument("--combine_contig", type=str, default=None, help="--combine_ref: only this contig")
    f.set_defaults(func=main_call_freq)
    # `combine_strands`: the last step -- the '-' strand row of each CpG folded onto the '+' strand cytosine, CGs of the genome
    # only (the reference's scripts/combine_two_strands_frequency.py; same flags, plus -o / --on / --device)
    from .combine_strands import add_arguments as combine_arguments
    c = sub.add_parser("combine_strands", description="combine the modification frequency of CG in the forward and backward strand")
    combine_arguments(c)
    c.set_defaults(func=main_combine_strands)
    parser.combine_parser = c
    # `evaluate`: the step that judges a set of calls -- accuracy and AUROC from the call_mods results of an unmethylated and a
    # fully methylated sample (the reference's scripts/evaluate_mods_call.py; same flags, plus --on / --device / --num_sites / --seed)
    from .evaluate_mods_call import add_arguments as evaluate_arguments
    v = sub.add_parser("evaluate", description="calculate call accuracy stats of call_mods results for methylated and unmethylated samples")
    evaluate_arguments(v)
    v.set_defaults(func=main_evaluate)
    parser.evaluate_parser = v
    # `denoise`: the training-side module -- false positive samples of a training file filtered by cross-ranking, the models trained
    # on the GPU (the reference's flags and defaults, deepsignal.py:389-418, plus --seed / --device / --scores_file)
    from .denoise import add_arguments as denoise_arguments
    d = sub.add_parser("denoise", description="denoise training samples by deep-learning, filter false positive samples")
    denoise_arguments(d)
    d.set_defaults(func=main_denoise)
    parser.denoise_parser = d
    # `train`: fit the BiLSTM variants (--is_cnn no) or the signal model alone (--is_rnn no) on the GPU and save TF checkpoints (the reference's flags and defaults,
    # train_model.py:288-346, plus --seed / --device)
    from .train_model import SCOPE_NOTE, add_arguments as train_arguments
    t = sub.add_parser("train", description="train a model, need two independent datasets for training and validating. " + SCOPE_NOTE)
    train_arguments(t)
    t.set_defaults(func=main_train)
    parser.train_parser = t
    return parser


def main(argv=None):
    parser = build_parser(_names_freq_file(sys.argv[1:] if argv is None else argv))
    args = parser.parse_args(argv)
    if not getattr(args, "func", None):
        parser.print_help()
        return 1
    if args.module == "call_mods":
        from .call_modifications import check_recheck_args
        try:
            check_recheck_args(args.precision, args.recheck_margin, args.recheck_precision)
        except ValueError as exc:
            parser.error(str(exc))
        sub = parser.call_mods_parser
        if args.result_file is None and args.freq_file is None:      # "--freq_f" given as another flag's value
            sub.error("the following arguments are required: --result_file/-o")
        if args.freq_file is None and (args.freq_bed or args.freq_sort or args.freq_prob_cf != 0.0 or args.freq_device is not None):
            sub.error("--freq_bed / --freq_sort / --freq_prob_cf / --freq_device need --freq_file")
        if args.freq_file is not None:
            from .call_modifications import FreqFileError, _check_freq_file
            if args.freq_prob_cf != args.freq_prob_cf:
                sub.error("--freq_prob_cf must be a number")
            if args.freq_device is not None and args.freq_device < 0:
                sub.error("--freq_device must be >= 0")
            try:
                _check_freq_file(None, False)
            except ValueError as exc:
                sub.error(str(exc))
            try:
                args.func(args)
            except FreqFileError as exc:
                print(str(exc), file=sys.stderr)
                return 1
            return 0
    if args.module == "combine_strands":
        from .combine_strands import check_arguments
        check_arguments(parser.combine_parser, args)
        return args.func(args)
    if args.module == "evaluate":
        from .evaluate_mods_call import check_arguments
        check_arguments(parser.evaluate_parser, args)
        return args.func(args)
    if args.module == "denoise":
        from .denoise import check_arguments
        check_arguments(parser.denoise_parser, args)
        return args.func(args)
    if args.module == "train":
        from .train_model import check_arguments
        check_arguments(parser.train_parser, args)
        return args.func(args)
    if args.module == "call_freq":
        return args.func(args)       # the script's own main: it validates the forwarded flags and returns the exit status
    args.func(args)
    return 0


if __name__ == "__main__":
    sys.exit(main())
