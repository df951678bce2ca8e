"""vcf-vaf-counter fixtures: the small inputs of tests/golden/vcf, the cases run
on them, and a Python statement of the contract of include/vafc.h (items 1-9)
over raw bytes.  The statement is what the tests compare everything else with:
the goldens of the reference binary show that it is the reference's behaviour,
the library and the kernel are then compared with it line for line."""
import gzip
import hashlib
import re
import struct
import zlib

I32_MISSING = -(1 << 31)
I32_VEND = -(1 << 31) + 1
HT_FLAG, HT_INT, HT_REAL, HT_STR = 0, 1, 2, 3
SKIP, SET, END, ABORT = 0, 1, 2, 3

# --------------------------------------------------------------------------
# the statement
# --------------------------------------------------------------------------


def load_patterns(data: bytes):
    """load_patterns: fscanf("%255s%d%d%255s %c %c%127s%127s") until a record
    does not convert; rows of (chr, start, rsid, ref, alt), bytes and ints."""
    tok = data.split()
    rows = []
    for i in range(0, len(tok) - 7, 8):
        t = tok[i:i + 8]
        if not re.fullmatch(rb"[+-]?\d+", t[1]) or not re.fullmatch(rb"[+-]?\d+", t[2]):
            break
        if len(t[4]) != 1 or len(t[5]) != 1:
            break
        rows.append((t[0], int(t[1]), t[3], t[4], t[5]))
    return rows


def write_vaf(rows, counts):
    """vc_write_vaf / vcf-vaf-counter.c:246-273; counts[i] = (ref, alt) as
    uint32.  Returns (the file's bytes, the average depth)."""
    tot = sum(r + a for r, a in counts)
    out = [b"# Average depth: %.2f\n" % (tot / (len(rows) if rows else 1)),
           b"CHR\tPOS\tRSID\tREF\tALT\tREF_COUNT\tALT_COUNT\tTOTAL_COUNT\tVAF\n"]
    for (c, s, rs, ref, alt), (r, a) in zip(rows, counts):
        total = (r + a) & 0xFFFFFFFF
        out.append(b"%s\t%d\t%s\t%s\t%s\t%d\t%d\t%d\t%.4f\n" % (c, s, rs, ref, alt, r, a, total, a / total if total else 0.0))
    return b"".join(out), tot / (len(rows) if rows else 1)


def find_pattern(rows, chrom: bytes, pos: int):
    """find_pattern (:83-92): the first row, or -1."""
    for i, r in enumerate(rows):
        if r[0] == chrom and r[1] == pos:
            return i
    return -1


def text_of(data: bytes):
    """Item 9: gzip and BGZF are inflated member by member; None for BCF."""
    if data[:2] == b"\x1f\x8b":
        out = []
        while data[:2] == b"\x1f\x8b":
            d = zlib.decompressobj(31)
            try:
                out.append(d.decompress(data))
            except zlib.error:
                break
            if not d.eof:
                break
            data = d.unused_data
        data = b"".join(out)
    return None if data[:3] == b"BCF" else data


def parse_header(text: bytes):
    """(n_samples, {FORMAT id: type}, offset of the body) or None (item 8)."""
    if text[:16] != b"##fileformat=VCF":
        return None
    types, p = {}, 0
    while True:
        if p >= len(text):
            return None
        nl = text.find(b"\n", p)
        end, nxt = (nl, nl + 1) if nl >= 0 else (len(text), len(text))
        line = text[p:end]
        if line.endswith(b"\r"):
            line = line[:-1]
        if not line:
            p = nxt
            continue
        if line[:1] != b"#":
            return None
        if line[:2] == b"##":
            m = re.fullmatch(rb"##FORMAT=<(.*)>[^>]*", line)
            if m:
                kv = dict(re.findall(rb'(?:^|,)([^=,]+)=("(?:[^"\\]|\\.)*"|[^,]*)', m.group(1))[::-1])
                t = {b"Integer": HT_INT, b"Float": HT_REAL, b"String": HT_STR, b"Character": HT_STR,
                     b"Flag": HT_FLAG}.get(kv.get(b"Type"))
                if kv.get(b"ID") and t is not None:
                    types.setdefault(kv[b"ID"], t)
            p = nxt
            continue
        if line[:7] not in (b"#CHROM\t", b"#CHROM "):
            return None
        tabs = line.count(b"\t")
        return (tabs - 8 if tabs >= 9 else 0), types, nxt


def _uint(s: bytes, i: int):
    """[+]digits at s[i:]: (value, index behind)."""
    if s[i:i + 1] == b"+":
        i += 1
    j = i
    while 48 <= s[j] <= 57:
        j += 1
    return (int(s[i:j]) if j > i else 0), j


def eval_line(hdr, line: bytes, sample_idx: int, min_depth: int):
    """One data line: a dict with head_ok, chrom, pos (POS - 1), n_allele, ref,
    alt (the REF and first ALT strings) and verdict SKIP / (SET, ref, alt) / END /
    ABORT, the verdict as if the line had hit a row and passed item 3."""
    n_samples, types, _ = hdr
    if line.endswith(b"\n"):
        line = line[:-1]
    if line.endswith(b"\r"):
        line = line[:-1]
    if b"\0" in line:
        line = line[:line.index(b"\0")]
    col = line.split(b"\t", 9)
    r = {"head_ok": False, "verdict": END, "chrom": col[0]}
    if len(col) < 6:                        # an empty CHROM is a contig like any other
        return r
    m = re.fullmatch(rb"\+?(\d*)", col[1])
    if not m or int(m.group(1) or b"0") >= 1 << 62:
        return r
    r.update(head_ok=True, pos=int(m.group(1) or b"0") - 1, ref=col[3])
    if col[4] == b".":
        r.update(n_allele=1, alt=b"")
    else:
        r.update(n_allele=2 + col[4].count(b","), alt=col[4].split(b",")[0])
    if len(col) < 8:
        return r
    r["verdict"] = SKIP
    if len(col) == 8 or n_samples == 0:
        return r
    if len(col) == 9 or col[8] == b".":     # vcf.c:3349-3350 turns "no sample columns" into success
        return r
    tags = col[8].split(b":")
    if len(tags) > 255 or b"." in tags:   # an empty tag is an undeclared one
        r["verdict"] = END
        return r
    ftype = [types.get(t, HT_STR) for t in tags]
    is_gt = [t == b"GT" for t in tags]
    dup = [t in tags[:j] for j, t in enumerate(tags)]
    # the widths over the first n_samples columns (vcf_parse_format_max3)
    cols = col[9].split(b"\t")
    if cols and cols[-1] == b"":
        cols.pop()                      # nothing behind the last tab: no column
    cols = cols[:n_samples]
    max_m, max_g = [0] * len(tags), [0] * len(tags)
    for c in cols:
        fields = c.split(b":")
        if len(fields) > len(tags):
            r["verdict"] = END
            return r
        for j, f in enumerate(fields):
            max_m[j] = max(max_m[j], 1 + f.count(b","))
            if is_gt[j]:
                max_g[j] = max(max_g[j], 1 + f.count(b"/") + f.count(b"|"))
    if HT_FLAG in ftype:
        r["verdict"] = END
        return r
    width = [(max_g[j] if is_gt[j] else 0) if ftype[j] == HT_STR else max(max_m[j], 1) for j in range(len(tags))]
    vals = [[] for _ in tags]
    # the values (vcf_parse_format_fill5); a column is parsed as a NUL-terminated string
    body = b"\0".join(cols)
    end = len(body) + (1 if len(col[9]) > len(body) else 0)   # the line goes on behind these columns
    s = body + b"\0\0\0\0"
    t, m_i = 0, 0
    while t < end and m_i < len(cols):
        j = 0
        while t < end:
            z = j
            j += 1
            x = []
            if dup[z]:
                while s[t] not in (58, 0):
                    t += 1
            elif ftype[z] == HT_STR:
                if is_gt[z]:
                    phased, unreadable = 0, False
                    while True:
                        if s[t] == 46:
                            t += 1
                            x.append(phased)
                        else:
                            if 48 <= s[t] <= 57 and not 48 <= s[t + 1] <= 57:
                                v, t = s[t] - 48, t + 1
                            else:
                                t0 = t
                                v, t = _uint(s, t)
                                v &= 0xFFFFFFFF
                                unreadable = unreadable or t == t0
                            if v > (1 << 30) - 2:
                                unreadable = True
                            x.append(((v + 1) << 1 | phased) & 0xFFFFFFFF)
                        phased = int(s[t] == 124)
                        if s[t] not in (124, 47):
                            break
                        t += 1
                    if unreadable:
                        r["verdict"] = END
                        return r
                    x = [v - (1 << 32) if v >= 1 << 31 else v for v in x]
                    x += [I32_VEND] * (width[z] - len(x))
                else:
                    while s[t] not in (58, 0):
                        t += 1
            elif ftype[z] == HT_INT:
                while True:
                    if s[t] == 46:
                        x.append(I32_MISSING)
                        t += 1
                    else:
                        mm = re.match(rb"[+-]?\d*", s[t:])
                        g = mm.group()
                        v = None if g == b"" else 0 if g in (b"+", b"-") else int(g)   # hts_str2int
                        if v is None or v < -2147483640 or v > 2147483647:
                            v = I32_MISSING
                        x.append(v)
                        t += mm.end()
                    if s[t] != 44:
                        break
                    t += 1
                x += [I32_VEND] * (width[z] - len(x))
            else:
                while True:
                    if s[t] == 46 and not 48 <= s[t + 1] <= 57:
                        t += 1
                    else:
                        mm = re.match(rb"[+-]?(\d+\.?\d*([eE][+-]?\d+)?|\.\d+([eE][+-]?\d+)?|inf(inity)?|nan)?", s[t:], re.I)
                        t += mm.end()
                    if s[t] != 44:
                        break
                    t += 1
            vals[z].append(x)
            if s[t] == 0:
                break
            if s[t] == 58:
                t += 1
            else:
                r["verdict"] = END
                return r
        for z in range(j, len(tags)):
            vals[z].append(([I32_MISSING] + [I32_VEND] * (width[z] - 1)) if width[z] else [])
        m_i += 1
        t += 1
    if len(cols) != n_samples:
        r["verdict"] = END
        return r
    # process_vcf :137-195
    def flat(tag, need_type):
        if tag not in tags:
            return None
        j = tags.index(tag)
        if ftype[j] != need_type:
            return None
        return [v for x in vals[j] for v in (x + [0] * width[j])[:width[j]]]
    s_i = sample_idx
    gt = flat(b"GT", HT_STR)
    if gt is not None and width[tags.index(b"GT")] == 0:
        r["verdict"] = ABORT             # GT in no sample column: bcf_get_format_values calls exit(1)
        return r
    if s_i < 0:
        return r
    if not gt or 2 * s_i + 1 >= len(gt):
        return r
    a1, a2 = (gt[2 * s_i] >> 1) - 1, (gt[2 * s_i + 1] >> 1) - 1
    if a1 < 0 or a2 < 0:
        return r
    depth = ref_d = alt_d = 0
    ad = flat(b"AD", HT_INT)
    if ad and 2 * s_i + 1 < len(ad) and ad[2 * s_i] != I32_MISSING and ad[2 * s_i + 1] != I32_MISSING:
        ref_d, alt_d = ad[2 * s_i], ad[2 * s_i + 1]
        depth = ((ref_d + alt_d + (1 << 31)) & 0xFFFFFFFF) - (1 << 31)
    if depth == 0:
        dp = flat(b"DP", HT_INT)
        if dp and s_i < len(dp) and dp[s_i] != I32_MISSING:
            depth = dp[s_i]
            if a1 == 0 and a2 == 0:
                ref_d, alt_d = depth, 0
            elif a1 == 1 and a2 == 1:
                ref_d, alt_d = 0, depth
            else:
                ref_d = int(depth / 2)      # C division truncates
                alt_d = depth - ref_d
    if depth < min_depth:
        return r
    r["verdict"] = (SET, ref_d & 0xFFFFFFFF, alt_d & 0xFFFFFFFF)
    return r


def to_start(pos: int) -> int:
    """(int)(POS - 1)."""
    return ((pos + (1 << 31)) & 0xFFFFFFFF) - (1 << 31)


def line_hit(rows, ev):
    """Items 2 and 3 for an evaluated line: the row it sets, or -1."""
    if not ev["head_ok"]:
        return -1
    i = find_pattern(rows, ev["chrom"], to_start(ev["pos"]))
    if i < 0 or ev["n_allele"] != 2 or len(ev["ref"]) != 1 or len(ev["alt"]) != 1:
        return -1
    return i if (ev["ref"], ev["alt"]) == (rows[i][3], rows[i][4]) else -1


def body_lines(text: bytes, start: int):
    """(offset, line) of every line from `start` on; the last needs no newline."""
    p = start
    while p < len(text):
        nl = text.find(b"\n", p)
        e = nl + 1 if nl >= 0 else len(text)
        yield p, text[p:e]
        p = e


def process_vcf(rows, data, sample_idx: int, min_depth: int):
    """process_vcf: (counts [(ref, alt)] per row, its Error: line or None)."""
    counts = [(0, 0)] * len(rows)
    if data is None:
        return counts, "open"
    text = text_of(data)
    hdr = parse_header(text) if text is not None else None
    if hdr is None:
        return counts, "header"
    for _, line in body_lines(text, hdr[2]):
        ev = eval_line(hdr, line, sample_idx, min_depth)
        if not ev["head_ok"]:
            break
        i = line_hit(rows, ev)
        if i < 0:
            continue
        if ev["verdict"] == ABORT:
            return counts, "abort"
        if ev["verdict"] == END:
            break
        if ev["verdict"] != SKIP:
            counts[i] = ev["verdict"][1:]
    return counts, None


def first_rows(rows) -> dict:
    """(chr, start) -> the first row that has them: find_pattern as a lookup."""
    index = {}
    for i, r in enumerate(rows):
        index.setdefault((r[0], r[1]), i)
    return index


def device_lines(rows, text: bytes, file_off: int = 0, index=None):
    """What the kernel reports for a block of complete lines: [(offset, row)],
    row -1 for a line it leaves to the host.  index: first_rows(rows), for
    large panels."""
    out = []
    for off, line in body_lines(text, 0):
        if line.endswith(b"\n"):
            line = line[:-1]
        col = line.split(b"\t")
        head = col[:5]
        if (len(col) < 6 or any(c < 32 for f in head for c in f) or not 0 < len(col[0]) <= 255   # the device's rule
                or not re.fullmatch(rb"\d{1,18}", col[1])):
            out.append((file_off + off, -1))
            continue
        if len(col[3]) != 1 or len(col[4]) != 1 or col[4] in (b".", b","):
            continue
        start = to_start(int(col[1]) - 1)
        i = find_pattern(rows, col[0], start) if index is None else index.get((col[0], start), -1)
        if i >= 0 and (col[3], col[4]) == (rows[i][3], rows[i][4]):
            out.append((file_off + off, i))
    return out


def synth_vcf(rows, n_lines: int, n_samples: int = 1, seed: int = 1, hit_rate: float = 0.004, header_too: bool = True):
    """Seeded WGS-shaped VCF text: n_lines records over the chromosomes of
    `rows` ((chr, start, rsid, ref, alt) as load_patterns gives them) in
    ascending position; about hit_rate of them sit on a row with its alleles,
    as many on a row with other alleles, the rest on positions of their own
    (some of them indels).  Sample columns are GT:AD:DP."""
    import numpy as np
    rng = np.random.default_rng(seed)
    n_rows = len(rows)
    kind = rng.random(n_lines)
    pick = rng.integers(0, max(n_rows, 1), n_lines)
    pos = np.sort(rng.integers(1, 240_000_000, n_lines))
    chroms = sorted({r[0] for r in rows}) or [b"chr1"]
    chrom_of = rng.integers(0, len(chroms), n_lines)
    bases = [b"A", b"C", b"G", b"T"]
    b1 = rng.integers(0, 4, n_lines)
    b2 = rng.integers(1, 4, n_lines)
    ad = rng.integers(0, 60, (n_lines, 2))
    gts = [b"0/0", b"0/1", b"1/1", b"0|1", b"./."]
    gt = rng.integers(0, len(gts), n_lines)
    out = [header(samples=["S%d" % i for i in range(n_samples)]).encode()] if header_too else []
    for i in range(n_lines):
        if n_rows and kind[i] < 2 * hit_rate:
            r = rows[pick[i]]
            c, p1, ref, alt = r[0], r[1] + 1, r[3], r[4]
            if kind[i] >= hit_rate:                 # the row's position with other alleles
                ref, alt = alt, ref
        else:
            c, p1 = chroms[chrom_of[i]], int(pos[i])
            ref, alt = bases[b1[i]], bases[(b1[i] + b2[i]) % 4]
            if kind[i] > 0.9:
                alt = alt + ref + ref               # an insertion
        one = b"%s:%d,%d:%d" % (gts[gt[i]], ad[i, 0], ad[i, 1], ad[i, 0] + ad[i, 1])
        out.append(b"%s\t%d\t.\t%s\t%s\t%d\tPASS\tAC=1;AN=2\tGT:AD:DP" % (c, p1, ref, alt, 30 + i % 60)
                   + (b"\t" + one) * n_samples + b"\n")
    return b"".join(out)


def c_atoi(s: str) -> int:
    m = re.match(r"\s*([+-]?\d+)", s)
    return to_start(int(m.group(1))) if m else 0


def run_statement(argv, read_file, writable=lambda name: True):
    """The whole command on argv (after the program name): (exit code, its own
    stderr text, the .vaf bytes or None).  read_file(name) -> bytes or None;
    writable(name): the output file can be created."""
    opts, i = {}, 0
    words = list(argv)
    while i < len(words):       # ketopt: every option here takes an argument, words are permuted
        w = words[i]
        if w.startswith("-") and len(w) > 1 and w[1] in "povsd":
            if len(w) > 2:
                opts[w[1]] = w[2:]
            elif i + 1 < len(words):
                i += 1
                opts[w[1]] = words[i]
        i += 1
    sample_idx = c_atoi(opts["s"]) if "s" in opts else 0
    min_depth = c_atoi(opts["d"]) if "d" in opts else 1
    if not all(k in opts for k in "pov"):
        return 1, ("Usage: vcf-vaf-counter [options] -p <patterns.txt> -v <input.vcf> -o <output.vaf>\nOptions:\n"
                   "  -p FILE   input pattern file\n  -v FILE   input VCF/BCF file\n  -o FILE   output VAF file\n"
                   "  -s INT    sample index (0-based) [%d]\n  -d INT    minimum depth [%d]\n" % (sample_idx, min_depth)), None
    err = "[M::main] Loading patterns...\n"
    pat = read_file(opts["p"])
    if pat is None:
        return 1, err + "Error: failed to load pattern file\n", None
    rows = load_patterns(pat)
    err += "[M::main] Loaded %d patterns\n[M::main] Processing VCF file...\n" % len(rows)
    counts, why = process_vcf(rows, read_file(opts["v"]), sample_idx, min_depth)
    if why == "open":
        err += "Error: failed to open VCF file: %s\n" % opts["v"]
    elif why == "header":
        err += "Error: failed to read VCF header\n"
    elif why == "abort":
        return 1, err, None
    err += "[M::main] Writing VAF file...\n"
    vaf, avg = write_vaf(rows, counts)
    if not writable(opts["o"]):
        return 1, err + "Error: failed to open output file\n", None
    return 0, err + "[M::main] Done. Average depth: %.2f\n" % avg, vaf


# --------------------------------------------------------------------------
# the inputs of tests/golden/vcf
# --------------------------------------------------------------------------

def bgzf(data: bytes, block: int = 400) -> bytes:
    """BGZF: gzip members with a BC extra field, then the empty EOF block."""
    out = []
    for i in list(range(0, len(data), block)) + [None]:
        raw = b"" if i is None else data[i:i + block]
        c = zlib.compressobj(6, zlib.DEFLATED, -15)
        comp = c.compress(raw) + c.flush()
        out.append(struct.pack("<4BI2BH2BHH", 31, 139, 8, 4, 0, 0, 255, 6, 66, 67, 2, len(comp) + 25) + comp
                   + struct.pack("<II", zlib.crc32(raw), len(raw)))
    return b"".join(out)


def header(samples=("S0", "S1"), gt="String", ad="Integer", dp="Integer", extra=()):
    h = ["##fileformat=VCFv4.2", "##contig=<ID=chr1,length=100000>", "##contig=<ID=chr2,length=100000>",
         "##contig=<ID=chr10,length=100000>"]
    if gt:
        h.append('##FORMAT=<ID=GT,Number=1,Type=%s,Description="Genotype">' % gt)
    if ad:
        h.append('##FORMAT=<ID=AD,Number=R,Type=%s,Description="Allelic depths, ref and alt">' % ad)
    if dp:
        h.append('##FORMAT=<ID=DP,Number=1,Type=%s,Description="Read depth">' % dp)
    h.extend(extra)
    h.append("#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO" + ("\tFORMAT\t" + "\t".join(samples) if samples else ""))
    return "\n".join(h) + "\n"


def rec(chrom, pos, ref, alt, fmt=None, *samples, id_=".", tail=".\t.\t."):
    s = "%s\t%s\t%s\t%s\t%s\t%s" % (chrom, pos, id_, ref, alt, tail)
    if fmt is not None:
        s += "\t" + fmt + "".join("\t" + x for x in samples)
    return s + "\n"


PANEL_ROWS = [
    ("chr1", 99, "rsA", "A", "C"), ("chr1", 99, "rsAdup", "A", "C"), ("chr1", 199, "rsB", "G", "T"),
    ("chr2", 9, "rsC", "C", "T"), ("chr1", 299, "rsD", "A", "G"), ("chr1", 399, "rsE", "T", "C"),
    ("chr1", 499, "rsF", "A", "C"), ("chrX", 0, "rsG", "A", "C"), ("chr1", 599, "rsH", "A", "C"),
    ("chr10", 99, "rsI", "A", "C"), ("chr1_x", 99, "rsJ", "A", "C"), ("chr1", -1, "rsK", "A", "C"),
    ("chr1", 699, "rsL", "A", "G"), ("chr1", 799, "rsM", "A", "C"), ("chr1", 799, "rsMdup", "G", "T"),
    ("chr1", 899, "rsN", "A", "C"), ("chr1", 999, "rsO", "A", "C"), ("chr1", 1099, "rsP", "A", "C"),
    ("chr1", 1199, "rsQ", "A", "C"), ("chr1", 1299, "rsR", "A", "C"), ("chr1", 1399, "rsS", "A", "C"),
    ("chr1", 1499, "rsT", "A", "C"), ("chr1", 1599, "rsU", "A", "C"), ("chr1", 1699, "rsV", "A", "C"),
    ("chr1", 1799, "rsW", "A", "C"), ("chr1", 1899, "rsX", "A", "C"), ("chr1", 1999, "rsY", "A", "C"),
]


def panel_text() -> str:
    return "".join("%s\t%d\t%d\t%s\t%s\t%s\tAAA\tACA\n" % (c, s, s + 1, rs, r, a) for c, s, rs, r, a in PANEL_ROWS)


def early_end(bad: str, **hdr) -> str:
    """A file that ends early: a hit, the line that stops it, a hit behind it."""
    return (header(**hdr) + rec("chr1", 100, "A", "C", "GT:AD", "0/1:3,4", "0/1:5,6") + bad
            + rec("chr1", 1000, "A", "C", "GT:AD", "0/1:30,40", "0/1:50,60"))


def inputs() -> dict:
    """name -> bytes of every input file."""
    F = {}
    F["p.txt"] = panel_text()
    F["p_empty.txt"] = ""
    F["main.vcf"] = header() + "".join([
        rec("chr1", 100, "A", "C", "GT:AD:DP", "0/1:10,5:15", "1/1:0,7:7"),      # the duplicate row stays 0 0
        rec("chr10", 100, "A", "C", "GT:AD", "0/1:1,2", "0/1:3,4"),
        rec("chr1_x", 100, "A", "C", "GT:AD", "0/1:5,6", "0/1:7,8"),             # not in the header
        rec("chrX", 1, "A", "C", "GT:AD", "0/1:1,1", "0/1:2,2"),                 # not in the header
        rec("chr1", 0, "A", "C", "GT:AD", "0/1:9,1", "0/1:1,9"),                 # start -1
        rec("chr1", "00200", "G", "T", "GT:DP", "0/0:8", "0/1:9"),               # leading zeros
        rec("chr1", (1 << 32) + 300, "A", "G", "GT:AD", "0|1:21,22", "1|0:23,24"),   # (int) truncates to 299
        rec("chr1", 400, "t", "c", "GT:AD", "0/1:9,9", "0/1:9,9"),               # lower case
        rec("chr1", 500, "A", ".", "GT:AD", "0/0:9,9", "0/0:9,9"),               # one allele
        rec("chr1", 600, "A", "C,G", "GT:AD", "0/1:1,1,1", "0/1:2,2,2"),         # three alleles
        rec("chr1", 700, "A", "G", "GT:AD", "0/1:3,4", "0/1:30,40"),
        rec("chr1", 700, "A", "G", "GT:AD", "0/1:6,1", "0/1:60,10"),             # the last qualifying record wins
        rec("chr1", 700, "A", "G", "GT:AD", "./.:9,9", "./.:9,9"),
        rec("chr1", 800, "G", "T", "GT:AD", "0/1:9,9", "0/1:9,9"),               # the first row is A C: no fall-through
        rec("chr1", "+900", "A", "C", "GT:AD", "0/1:11,12", "0/1:13,14"),
        rec("chr1", 1000, "AT", "C", "GT:AD", "0/1:9,9", "0/1:9,9"),             # REF of two bytes
        rec("chr3", 100, "A", "C", "GT:AD", "0/1:9,9", "0/1:9,9", id_="rs" + "x" * 300),
    ])
    F["main.vcf.gz"] = None     # gzip of main.vcf, made below
    F["gt.vcf"] = header() + "".join([
        rec("chr1", 100, "A", "C", "GT:AD", "1:2,3", "0:4,5"),                   # haploid: sample 0 gets both
        rec("chr1", 200, "G", "T", "GT:DP", "0/1/1:12", "0/0/1:14"),             # triploid shifts sample 1
        rec("chr1", 300, "A", "G", "GT:AD", ".|1:5,5", "0/.:6,6"),
        rec("chr1", 700, "A", "G", "GT:AD", "0|1:7,8", "1/1:9,10"),
        rec("chr1", 900, "A", "C", "GT:AD", "0/1:1,2", "1:3,4"),                 # a padding entry for sample 1
        rec("chr1", 1100, "A", "C", "AD", "1,2", "3,4"),                         # no GT
        rec("chr1", 1200, "A", "C", "AD:GT", "1,2", "3,4:0/1"),                  # GT left out for sample 0
        rec("chr1", 1300, "A", "C", "."),
    ])
    F["gt_int.vcf"] = early_end(rec("chr1", 200, "G", "T", "GT:AD", "0/1:1,2", "0/1:3,4"), gt="Integer")
    F["ad.vcf"] = header() + "".join([
        rec("chr1", 100, "A", "C", "GT:AD", "0/1:1,2,3", "0/1:4,5,6"),           # three values: sample 1 reads 3,4
        rec("chr1", 200, "G", "T", "GT:AD:DP", "0/1:5:11", "0/1:7:13"),          # one value: sample 0 reads 5,7
        rec("chr1", 300, "A", "G", "GT:AD:DP", "0/1:.,4:15", "1|1:3,.:13"),      # missing: DP instead
        rec("chr1", 700, "A", "G", "GT:AD:DP", "0/1:5:9", "0/1:7,8:9"),          # sample 0: 5 and the vector end
        rec("chr1", 900, "A", "C", "GT:AD:DP", "0/1:0,0:15", "0/0:0,0:9"),       # AD 0,0: DP is tried
        rec("chr1", 1100, "A", "C", "GT:AD:DP", "0/1:.:.", "0/1:.:."),
    ])
    F["noad.vcf"] = header(ad=None) + rec("chr1", 100, "A", "C", "GT:AD:DP", "0/1:10,5:15", "1/1:0,7:7")
    F["dp.vcf"] = header() + "".join([
        rec("chr1", 100, "A", "C", "GT:DP", "0/1:15", "0/1:9"),
        rec("chr1", 200, "G", "T", "GT:DP", "1|1:13", "0/0:21"),
        rec("chr1", 300, "A", "G", "GT:DP", "1/0:1", "0/2:7"),
        rec("chr1", 700, "A", "G", "GT:DP", "0/1:.", "0/1"),
        rec("chr1", 900, "A", "C", "GT:XX:DP", "0/1:a,b:6", "0/1:c:8"),
    ])
    F["dp_str.vcf"] = header(dp="String") + rec("chr1", 100, "A", "C", "GT:DP", "0/1:15", "0/1:9")
    F["depth.vcf"] = header() + "".join([
        rec("chr1", 100, "A", "C", "GT:AD", "0/1:3,3", "0/1:4,4"),               # depth 6 and 8 around -d 7
        rec("chr1", 200, "G", "T", "GT:AD", "0/1:3,4", "0/1:5,6"),
        rec("chr1", 200, "G", "T", "GT:AD", "0/1:0,0", "0/1:1,0"),               # -d 0: depth 0 sets 0 0
        rec("chr1", 300, "A", "G", "GT:DP", "0/1:7", "0/1:6"),
    ])
    F["end_pos.vcf"] = early_end(rec("chr7", "12x", "A", "C", "GT", "0/1", "0/1"))
    F["end_empty.vcf"] = early_end("\n")
    F["end_hash.vcf"] = early_end("#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tS0\tS1\n")
    F["end_ncols.vcf"] = early_end(rec("chr1", 200, "G", "T", "GT:AD", "0/1:1,2"))
    F["end_char.vcf"] = early_end(rec("chr1", 200, "G", "T", "GT:AD", "0/1:1,2x", "0/1:3,4"))
    F["end_short.vcf"] = early_end("chr1\t200\t.\tG\tT\t.\t.\n")
    F["nosample.vcf"] = early_end(rec("chr1", 200, "G", "T", "GT:AD"))
    F["end_fields.vcf"] = early_end(rec("chr1", 200, "G", "T", "GT:AD", "0/1:1,2:9", "0/1:3,4"))
    F["end_gt.vcf"] = early_end(rec("chr1", 200, "G", "T", "GT:AD", "0/x:1,2", "0/1:3,4"))
    F["end_tabs.vcf"] = early_end("chr9\t200\t.\tG\n")
    F["end_tagdot.vcf"] = early_end(rec("chr1", 200, "G", "T", "GT:.:DP", "0/1:x:5", "0/1:y:7"))
    FL = ('##FORMAT=<ID=FL,Number=0,Type=Flag,Description="A flag, which FORMAT cannot hold">',)
    F["end_flag.vcf"] = early_end(rec("chr1", 200, "G", "T", "GT:FL:DP", "0/1:x:5", "0/1:y:7"), extra=FL)
    F["end_tags256.vcf"] = early_end(rec("chr1", 200, "G", "T", ":".join(["GT"] + ["T%d" % i for i in range(255)]), "0/1", "0/1"))
    # lines that look wrong and end nothing: 255 tags, an empty CHROM, empty FORMAT tags, a last GT left empty
    F["goes_on.vcf"] = early_end(
        rec("chr1", 200, "G", "T", ":".join(["GT"] + ["T%d" % i for i in range(254)]), "0/1", "0/1")
        + "\t300\t.\tA\tG\t.\t.\t.\tGT:AD\t0/1:1,2\t0/1:3,4\n"
        + rec("chr1", 200, "G", "T", "GT::DP", "0/1:x:5", "0/1:y:7")
        + rec("chr1", 300, "A", "G", ":GT:AD:", "x:0/1:8,9", "y:1/1:10,11:z")
        + rec("chr1", 700, "A", "G", "DP:GT", "5:0/1", "7:"))
    F["abort_gt.vcf"] = early_end(rec("chr1", 200, "G", "T", "DP:GT", "5", "7"))
    F["abort_gt_nohit.vcf"] = early_end(rec("chr1", 200, "G", "A", "DP:GT", "5", "7") + rec("chr7", 200, "G", "T", "DP:GT", ".", "-3"))
    F["more_cols.vcf"] = header() + rec("chr1", 100, "A", "C", "GT:AD", "0/1:3,4", "0/1:5,6", "0/1:7,8")
    F["sites.vcf"] = header(samples=()) + rec("chr1", 100, "A", "C") + rec("chr1", 200, "G", "T")
    F["crlf.vcf"] = F["main.vcf"].replace("\n", "\r\n")
    F["nonl.vcf"] = (header() + rec("chr1", 100, "A", "C", "GT:AD", "0/1:3,4", "0/1:5,6")
                     + rec("chr1", 200, "G", "T", "GT:AD", "0/1:1,2", "0/1:3,4")[:-1])
    F["junk.vcf"] = "hello\nworld\n"
    F["nochrom.vcf"] = "##fileformat=VCFv4.2\n" + rec("chr1", 100, "A", "C")
    out = {k: (v.encode() if isinstance(v, str) else v) for k, v in F.items()}
    out["main.vcf.gz"] = gzip.compress(out["main.vcf"], mtime=0)
    out["main_bgzf.vcf.gz"] = bgzf(out["main.vcf"])
    return out


def cases() -> dict:
    """name -> argv (after the program name), run in a directory holding the
    inputs and an empty directory o/."""
    def A(vcf, *more, p="p.txt"):
        return ["-p", p, "-v", vcf, "-o", "o/out.vaf"] + list(more)
    c = {
        "main_s0": A("main.vcf"), "main_s1": A("main.vcf", "-s", "1"), "main_s_past": A("main.vcf", "-s", "2"),
        "main_gz": A("main.vcf.gz"), "main_bgzf": A("main_bgzf.vcf.gz", "-s1"), "crlf": A("crlf.vcf"), "nonl": A("nonl.vcf"),
        "nonl_s1": A("nonl.vcf", "-s", "1"),
        "gt_s0": A("gt.vcf"), "gt_s1": A("gt.vcf", "-s", "1"), "gt_int": A("gt_int.vcf"),
        "ad_s0": A("ad.vcf"), "ad_s1": A("ad.vcf", "-s", "1"), "noad_s0": A("noad.vcf"), "noad_s1": A("noad.vcf", "-s", "1"),
        "dp_s0": A("dp.vcf"), "dp_s1": A("dp.vcf", "-s", "1"), "dp_str": A("dp_str.vcf"),
        "depth_d7": A("depth.vcf", "-d", "7"), "depth_d7_s1": A("depth.vcf", "-d", "7", "-s", "1"),
        "depth_d0": A("depth.vcf", "-d", "0"), "depth_d0_s1": A("depth.vcf", "-d0", "-s1"), "depth_d1": A("depth.vcf"),
        "more_cols": A("more_cols.vcf", "-s", "1"), "nosample": A("nosample.vcf"), "sites": A("sites.vcf"),
        "junk": A("junk.vcf"), "nochrom": A("nochrom.vcf"), "missing_input": A("nope.vcf"),
        "missing_patterns": A("main.vcf", p="nope.txt"), "bad_outdir": ["-p", "p.txt", "-v", "main.vcf", "-o", "nodir/out.vaf"],
        "empty_patterns": A("main.vcf", p="p_empty.txt"),
        "opts_after_file": ["stray.vcf", "-s", "1", "-vmain.vcf", "-o", "o/out.vaf", "-pp.txt", "-d", "2"],
        "usage_no_v": ["-p", "p.txt", "-o", "o/out.vaf", "-s", "3", "-d", "9"],
    }
    c.update({"goes_on": A("goes_on.vcf"), "goes_on_s1": A("goes_on.vcf", "-s", "1"), "abort_gt": A("abort_gt.vcf"),
              "abort_gt_s_past": A("abort_gt.vcf", "-s", "9"), "abort_gt_nohit": A("abort_gt_nohit.vcf")})
    for k in ("pos", "empty", "hash", "ncols", "char", "short", "fields", "gt", "tabs", "tagdot", "flag", "tags256"):
        c["end_" + k] = A("end_%s.vcf" % k)
    return c


def vaf_entry(vaf: bytes) -> dict:
    lines = vaf.decode().splitlines()
    return {"md5": hashlib.md5(vaf).hexdigest(), "depth": lines[0],
            "counts": " ".join("%s %s" % tuple(ln.split("\t")[5:7]) for ln in lines[2:])}
