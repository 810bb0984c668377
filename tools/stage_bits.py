"""Two library builds (tools/ab_build.sh) compared bit for bit on the Forward, domain and alignment stages: a fresh
child process per library (MSV_LIB_PATH) runs the same seeded inputs and saves every output array as bytes.

    python tools/stage_bits.py ab/parent/libmsv_hip.so ab/branch/libmsv_hip.so [--out profiles/x.txt]

100.hmm under every variant (set_variant; the ...i ones on a profile made with insert odds) on the aimed batches of
tests/forward_batches.py and tests/decode_batches.py plus homologs of lengths 127-129 and ~400 (the rescale fires both
ways) and a bad residue; 600.hmm (S = 12, all 64 lanes, both insert modes), 1400.hmm and 2405.hmm on the automatic
variant with 32 homologs.  Forward's own call raises on a bad residue, so it scores the batch without it: fwd_kernel's
bad-residue path is compared only through the decode's forward scores."""
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def child(out):
    import hmm_fasta_viterbi_amd as msv
    from hmm_fasta_viterbi_amd.synthetic import concat_batches, gapped_homolog_batch, homolog_batch
    from decode_batches import region_batch
    from forward_batches import aimed_batch
    pairs = list(zip(msv.Forward_HMM.variants(), msv.Domain_HMM.variants()))
    runs = [("100.hmm", fv, dv, dv.endswith("i")) for fv, dv in pairs]
    runs += [("600.hmm", None, None, False), ("600.hmm", None, None, True), ("1400.hmm", None, None, False),
             ("2405.hmm", None, None, False)]
    got = {}
    for prof, fv, dv, ins in runs:
        h = msv.Profile_HMM(os.path.join(ROOT, "data", "profile_HMMs", prof))
        me = h.match_emissions
        parts = [homolog_batch(me, 60, 28, 300, 500), gapped_homolog_batch(me, 61, 4, 300, 500)]
        mode = msv.INSERTS_LOG_ODDS if ins else msv.INSERTS_ZERO
        fwd, dom = msv.Forward_HMM(h, insert_mode=mode), msv.Domain_HMM(h, insert_mode=mode)
        if fv:
            fwd.set_variant(fv)
            dom.set_variant(dv)
            model, S = (fwd.match_scores,), int(re.search(r"_s(\d+)", dv).group(1))
            parts = [aimed_batch(model, S, 900 + S)[0], region_batch(model, 720 + S)[0],
                     homolog_batch(me, 40, 6, 127, 129), homolog_batch(me, 50, 6, 380, 420),
                     gapped_homolog_batch(me, 51, 4, 380, 420)]
        codes, offsets = concat_batches(*parts)
        codes = codes.copy()
        codes[int(offsets[-2]) + 5] = 23  # a bad residue in the last sequence
        key = f"{prof}/{dv or 'auto' + 'i' * ins}/"
        clean = np.where(codes < 20, codes, 0).astype(np.uint8)
        got[key + "forward.scores"] = fwd.score_batch(codes=clean, offsets=offsets)
        e = dom.decode_batch(codes=codes, offsets=offsets, strict=False)
        for f in ("forward_scores", "backward_scores", "begin", "end", "occ", "regions"):
            got[key + "decode." + f] = getattr(e, f)
        al = dom.align_batch(codes=codes, offsets=offsets, envelopes=e, keep_posteriors=True, strict=False)
        for f in ("envelope_scores", "oa_scores", "domains", "ops", "op_pp"):
            got[key + "align." + f] = getattr(al, f)
        for j, name in enumerate(("ppM", "ppI", "ppN", "ppJ", "ppC")):
            got[key + "align." + name] = np.concatenate([np.zeros(0, np.float32)] + [al.posteriors(q)[j].ravel()
                                                                                    for q in range(len(al.items))])
        fwd.close()
        dom.close()
    np.savez(out, **{k: np.frombuffer(np.ascontiguousarray(v).tobytes(), np.uint8) for k, v in got.items()})


def main():
    if sys.argv[1] == "--child":
        return child(sys.argv[2])
    libs, out = sys.argv[1:3], sys.argv[4] if sys.argv[3:4] == ["--out"] else ""
    with tempfile.TemporaryDirectory() as tmp:
        for i, lib in enumerate(libs):
            subprocess.run([sys.executable, os.path.abspath(__file__), "--child", os.path.join(tmp, f"{i}.npz")],
                           env=dict(os.environ, MSV_LIB_PATH=os.path.abspath(lib)), check=True, timeout=900)
        x, y = (dict(np.load(os.path.join(tmp, f"{i}.npz"))) for i in range(2))
    assert x.keys() == y.keys()
    lines = [f"{k:44s} {x[k].size:10d} bytes  {'equal' if np.array_equal(x[k], y[k]) else 'DIFFERENT'}" for k in x]
    bad = sum(line.endswith("DIFFERENT") for line in lines)
    text = "\n".join([f"{libs[0]} against {libs[1]}: every output array as bytes"] + lines +
                     [f"arrays: {len(x)}, different: {bad}"]) + "\n"
    sys.stdout.write(text)
    if out:
        open(out, "w").write(text)
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
