"""``--trimmed-out [plain|gz]``: every sample's trimmed reads as FASTQ (FASTA, or one sequence per line), formatted on the device from the text
the parse already holds there.  The sentences below are the specification (tests/fq_restate.py restates them byte by byte).

The stream S of one sample
  Take the records of the sample's text in file order.  Record r is written if and only if its read after the LAST modifier of the chain
  (``-q``, ``-a`` / ``-g``, ``--trim-n``, ``-u``, ``-a auto``) has at least ``--minimum-length`` letters -- whatever ``--trim-count`` says: the
  written records are exactly the ``trimmed`` view of ``--read-qc``.  Without any modifier the read is the sequence line with a trailing
  ``\\r`` stripped.  With the read's bounds ``[ts, te)`` inside the sequence line ``[ls, le)`` and the quality line starting at ``qs``, the
  quality slice is ``text[qs + ts - ls : qs + te - ls]``.

  A written record, by input format as the parser numbers them:
    1 (FASTQ)                  ``H \\n S \\n + \\n Q \\n``: H the header line verbatim (the ``@`` included, a trailing ``\\r`` stripped), S =
                               ``text[ts:te]`` verbatim -- lower case, ``U``, IUPAC codes and ``.`` stay as they are --, the third line always a
                               bare ``+``, Q the quality slice
    2 (FASTA, after ``unwrap_fasta``)   ``H \\n S \\n``
    3 (one sequence per line)  ``S \\n``

  Line ends are ``\\n`` whatever the input used.  A kept read of length 0 (``-m 0``) writes its empty lines.  S depends only on the input and
  the options: not on how the sample was cut into pieces, not on chunk or tile sizes, not on timing.

Files
  plain   ``<sample>.trimmed.fastq``, ``.trimmed.fasta`` or ``.trimmed.txt`` by input format, holding S.
  gz      ``<name>.gz`` and ``<name>.gz.gzi``, BGZF exactly as mirge3_amd/bgzf.py specifies it: member b holds ``S[b*B:(b+1)*B]`` with B from
          ``MIRGE_BGZF_BLOCK_BYTES`` (default 65280), each member stored, fixed or dynamic by the rule given there, the EOF block behind the
          last member; an empty S is the EOF block alone with a ``.gzi`` of eight zero bytes.  Compressed offsets of the ``.gzi`` are file
          offsets, uncompressed offsets are stream offsets.  ``MIRGE_BGZF_DEFLATE=host`` is the A/B route, as for ``--bgzf-out``.
  All files are written as ``<name>.tmp`` and renamed when the sample's parse has ended without error; a failed run leaves no trimmed file
  of that sample.  With ``--kmer-correct`` the file holds the reads BEFORE correction.

Errors
  A FASTQ record whose quality line is not as long as its sequence line is an error: the parse's message, prefixed ``--trimmed-out:``, raised
  before that piece writes anything.  A piece writes only AFTER its reads were packed: a broken record structure, a letter that is no
  nucleotide code or a read that is too long never reaches the file.

run.log
  ``trimmed out <sample>: R records, W written, T too short, B bytes`` and with ``gz`` ``; F file bytes, M members (stored a, fixed b, dynamic c)``.

Device side: csrc/kernels_fq.hpp (k_fq_measure, k_fq_write), csrc/native_fq.hpp (``mirge_fqout``, ``mirge_reads_parse_trim_out``); sizes
``MIRGE_FQ_CHUNK_BYTES`` (default 32 MiB) and ``MIRGE_FQ_TILE_BYTES`` (a multiple of 16, at most 16384).
"""
from __future__ import annotations

import os

MODES = ("plain", "gz")
EXTENSIONS = {1: "fastq", 2: "fasta", 3: "txt"}


def file_name(sample: str, fmt: int, mode: str = "plain") -> str:
    """the file of ``sample`` for input format ``fmt`` (1 FASTQ, 2 FASTA, 3 one sequence per line); ``gz``: its ``.gzi`` is this name + ``.gzi``"""
    if mode not in MODES:
        raise ValueError(f"mode={mode!r}: plain or gz")
    return f"{sample}.trimmed.{EXTENSIONS[int(fmt)]}" + (".gz" if mode == "gz" else "")


def log_line(sample: str, stats: dict, mode: str = "plain") -> str:
    """the sample's run.log line from ``_ffi.TrimmedOut.finish()``"""
    line = (f"trimmed out {sample}: {stats['records']} records, {stats['written']} written, {stats['records'] - stats['written']} too short, "
            f"{stats['stream_bytes']} bytes")
    if mode == "gz":
        line += (f"; {stats['file_bytes']} file bytes, {stats['members']} members (stored {stats['stored']}, fixed {stats['fixed']}, "
                 f"dynamic {stats['dynamic']})")
    return line


def refusal(args) -> str:
    """Why this command line's ``--trimmed-out`` is refused, or "" (``cli.parse_args`` hands it to ``ap.error`` before anything is written).
    ``-a auto``, ``--read-qc``, ``--kmer-correct`` and every exporter are legal beside the flag."""
    mode = getattr(args, "trimmed_out", None)
    if not mode:
        return ""
    if mode not in MODES:
        return f"--trimmed-out {mode}: plain or gz"
    if getattr(args, "uniq_mol_ids", None):
        return "--trimmed-out: not together with -umi (the UMI routes slice the reads and take the sample whole)"
    if getattr(args, "save_pkl", False) or getattr(args, "resume", False) or getattr(args, "backend", "gpu") == "bowtie":
        return "--trimmed-out runs on the device-resident route: not together with -spl / -rr / --backend bowtie"
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        return "--trimmed-out is a single-process option"
    if mode == "gz":
        from . import bgzf
        try:
            bgzf.route()
            bgzf.block_bytes()
        except ValueError as e:
            return f"--trimmed-out gz: {e}"
    return ""
