"""Helpers of the --truth-tags GPU tests: tagged records split into the record truth_util.parse_record reads and the
tag bytes behind it, the reference as the model wants it, and the model (tests/tags_model.py) applied to every read of a
Session's pass."""
import re
import struct

import tags_model as TM
import truth_util as U


def config_value(cfg, key):
    return re.search(r"^%s = (\S+)" % key, open(cfg).read(), re.M).group(1)


def read_length(cfg):
    return int(re.search(r"readLength: (\d+)", open(config_value(cfg, "profile")).read()).group(1))


def fasta_sequences(path):
    """The contigs' bytes as the file holds them (either case, line ends taken out), in file order: index = BAM refID."""
    out = []
    for ln in open(path, "rb").read().split(b"\n"):
        if ln.startswith(b">"):
            out.append(bytearray())
        elif out:
            out[-1] += ln
    return [bytes(s) for s in out]


def raw_records(stream):
    """The records of a headerless record stream as bytes, each with its block_size word."""
    out, off = [], 0
    while off < len(stream):
        bs = struct.unpack_from("<I", stream, off)[0]
        out.append(stream[off:off + 4 + bs])
        off += 4 + bs
    assert off == len(stream)
    return out


def split_record(r):
    """(the record without its optional fields, block_size lowered to match; the optional fields' bytes)."""
    lname, ncig, lseq = r[12], struct.unpack_from("<H", r, 16)[0], struct.unpack_from("<I", r, 20)[0]
    front = 36 + lname + 4 * ncig + (lseq + 1) // 2 + lseq
    assert front <= len(r)
    return struct.pack("<I", front - 4) + r[4:front], r[front:]


def with_tags(plain, tag_bytes):
    """An untagged record with `tag_bytes` appended and block_size raised."""
    return struct.pack("<I", len(plain) - 4 + len(tag_bytes)) + plain[4:] + tag_bytes


def model_of_pass(sess, plain_records, paired, L, fastas, mask=TM.TAG_ALL, cap=2048):
    """The model's tags of every record of the pass just sampled, in record order: [(tags dict, MD dropped)].  The
    alignment comes from the untagged record, the template and the events from sg_truth_reads, the chains' codes from
    sg_haplotype_codes."""
    n = sess.batch_slots
    rows = [sess.truth_reads(m, 0, n) for m in range(2 if paired else 1)]
    out = []
    it = iter(plain_records)
    for t in range(n):
        for m in range(len(rows)):
            r = rows[m][t]
            if not r.live:
                continue
            rec = U.parse_record(next(it))
            _, read, _ = U.fastq_view(rec)
            assert len(read) == r.read_len
            codes = sess.haplotype_codes(r.chain, r.tmpl_off, L) if r.inside else None
            fasta = fastas[rec["rid"]] if rec["ops"] else b""
            out.append(TM.tags(rec["ops"], rec["seq"], fasta, rec["pos"], bool(r.inside), codes, bool(r.reverse),
                               [r.events[e] for e in range(r.n_events)], read, mask, cap) + (rec, r))
    assert next(it, None) is None, "more records than live reads"
    return out


def tagged_pass(sess, paired, L, fastas, mask=TM.TAG_ALL):
    """After sample() and result(): the untagged records, the tagged stream and the model's rows; asserts that the tagged
    stream is, byte for byte, the untagged records with block_size raised and the model's tag bytes behind them, that
    its BGZF members inflate to it, and that sg_truth_tag_info's sums are the model's."""
    rb, _ = sess.truth_bam()
    plain = raw_records(sess.fetch_truth(False, rb))
    rb, gb = sess.truth_bam(mask)
    stream = sess.fetch_truth(False, rb)
    assert U.inflate_members(sess.fetch_truth(True, gb), want_eof=False) == stream if rb else gb == 0
    info = sess.truth_tag_info()
    cap = int(info.max_md)
    model = model_of_pass(sess, plain, paired, L, fastas, mask, cap)
    want = [with_tags(p, TM.tag_bytes(t)) for p, (t, _, _, _) in zip(plain, model)]
    if stream != b"".join(want):
        got = raw_records(stream)
        assert len(got) == len(want), (len(got), len(want))
        for i, (g, w) in enumerate(zip(got, want)):
            assert g == w, (i, model[i][0], TM.parse_tags(split_record(g)[1]), model[i][2]["ops"], model[i][2]["pos"])
    assert sess.truth_info()[0] == len(plain)
    tags = [t for t, _, _, _ in model]
    assert (info.n_nm, info.n_md, info.n_xe) == tuple(sum(k in t for t in tags) for k in ("NM", "MD", "XE"))
    assert (info.nm_sum, info.xe_sum) == (sum(t.get("NM", 0) for t in tags), sum(t.get("XE", 0) for t in tags))
    assert info.md_dropped == sum(d for _, d, _, _ in model)
    assert info.tag_bytes == sum(len(TM.tag_bytes(t)) for t in tags) == len(stream) - sum(len(p) for p in plain)
    return plain, stream, model, info
