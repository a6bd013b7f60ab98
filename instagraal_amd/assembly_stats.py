"""N50 / L50 / N90 / L90, lengths and G+C of an assembly: the reference's ``assembly_stats`` restated.  The dict and
the two strings are the reference's, character for character; the numbers come either from a FASTA (plain or ``.gz``, read by
``pre.read_fasta``) or from the lengths and G+C counts somebody already has (``scaffold_polish.composition``, the device's counts)."""
import statistics

KEYS = ("n_contigs", "total_length", "largest_contig", "shortest_contig", "mean_length", "median_length", "n50", "l50", "n90", "l90", "gc_content")
_SINGLE = (("Sequences (contigs/scaffolds)", "n_contigs", "int"), ("Total length (bp)", "total_length", "int"), ("Largest sequence (bp)", "largest_contig", "int"),
           ("Shortest sequence (bp)", "shortest_contig", "int"), ("Mean length (bp)", "mean_length", "float"), ("Median length (bp)", "median_length", "float"),
           ("N50 (bp)", "n50", "int"), ("L50 (# sequences)", "l50", "int"), ("N90 (bp)", "n90", "int"), ("L90 (# sequences)", "l90", "int"))
_TABLE = (("Sequences", "n_contigs", "int"), ("Total length (bp)", "total_length", "int"), ("Largest (bp)", "largest_contig", "int"), ("Shortest (bp)", "shortest_contig", "int"),
          ("Mean length (bp)", "mean_length", "float"), ("Median length (bp)", "median_length", "float"), ("N50 (bp)", "n50", "int"), ("L50", "l50", "int"),
          ("N90 (bp)", "n90", "int"), ("L90", "l90", "int"), ("GC content", "gc_content", "pct"))


def lengths_and_gc(fasta_path):
    """-> (lengths, G+C counts) of the records of a FASTA, the empty ones left out as the reference leaves them out"""
    from .pre import read_fasta

    lengths, gc = [], []
    for _, seq in read_fasta(fasta_path):
        if len(seq):
            up = seq.upper()
            lengths.append(len(seq))
            gc.append(up.count(b"G") + up.count(b"C"))
    return lengths, gc


def nx_lx(lengths_desc, total, fraction):
    """the length at which the running sum of the lengths, longest first, reaches ``fraction`` of the total, and how many it took"""
    target, run = total * fraction, 0
    for k, n in enumerate(lengths_desc, start=1):
        run += n
        if run >= target:
            return n, k
    return lengths_desc[-1], len(lengths_desc)


def compute_assembly_stats(fasta_or_lengths, gc_counts=None):
    """``compute_assembly_stats(path)`` or ``compute_assembly_stats(lengths, gc_counts)`` -> the reference's dict (``KEYS``)"""
    if gc_counts is None:
        lengths, gc_counts = lengths_and_gc(fasta_or_lengths)
    else:
        keep = [(int(n), int(g)) for n, g in zip(fasta_or_lengths, gc_counts) if int(n) > 0]
        lengths, gc_counts = [n for n, _ in keep], [g for _, g in keep]
    if not lengths:
        return dict(n_contigs=0, total_length=0, largest_contig=0, shortest_contig=0, mean_length=0.0, median_length=0.0, n50=0, l50=0, n90=0, l90=0, gc_content=0.0)
    desc = sorted(lengths, reverse=True)
    total = sum(lengths)
    n50, l50 = nx_lx(desc, total, 0.50)
    n90, l90 = nx_lx(desc, total, 0.90)
    return dict(n_contigs=len(lengths), total_length=total, largest_contig=desc[0], shortest_contig=desc[-1], mean_length=total / len(lengths),
                median_length=statistics.median(lengths), n50=n50, l50=l50, n90=n90, l90=l90, gc_content=sum(gc_counts) / total)


def format_assembly_stats(stats, label=None):
    rule = "  " + "-" * 42
    lines = ["", "  %s" % label if label else "  Assembly statistics", rule]
    for text, key, kind in _SINGLE:
        lines.append("  %-34s " % text + (format(stats[key], ">7,") if kind == "int" else format(stats[key], ">10,.1f")))
    lines += ["  %-34s " % "GC content" + format(stats["gc_content"] * 100, ">9.2f") + "%", rule, ""]
    return "\n".join(lines)


def format_comparison_table(results):
    """``{label: stats}`` in the order of the columns -> the side-by-side table"""
    labels = list(results)
    col_w = max([14] + [len(lb) + 2 for lb in labels])
    metric_w = 22

    def cell(value, kind):
        if kind == "int":
            return format(int(value), ">%d," % col_w)
        if kind == "float":
            return format(value, ">%d,.1f" % col_w)
        return format(value * 100, ">%d.2f" % (col_w - 1)) + "%"

    rule = "  " + "-" * (metric_w + col_w * len(labels) + 2)
    rows = ["", "  Assembly statistics comparison", rule, "  " + "Metric".ljust(metric_w) + "".join(lb.rjust(col_w) for lb in labels), rule]
    for text, key, kind in _TABLE:
        rows.append("  " + text.ljust(metric_w) + "".join(cell(results[lb][key], kind) for lb in labels))
    return "\n".join(rows + [rule, ""])
