"""bench.py's plain run (no --full) and --dump-outputs: the K timed steps and nothing after them, and the proof of the last step written out as the prover returned it,
the same on every run with the same arguments."""
import glob, json, os, subprocess, sys, tempfile
import numpy as np
import pytest
from blockmaze_amd import engine as e
import workload as w
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

def run(args, timeout=600):
    env = dict(os.environ); env.pop("RANK", None); env.pop("WORLD_SIZE", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, capture_output=True, text=True, env=env, timeout=timeout)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]; assert len(lines) == 1, r.stdout[-500:]; return json.loads(lines[0])

def test_plain_run_dumps_the_proof_of_its_last_step(tmp_path):
    """the line of a plain run carries the headline and none of the --full legs; DIR/proof.npy holds the last timed step's proof (float64, one byte a value), equal to
    what the prover returns for that statement and (r, s) from a host buffer, accepted by the verifier, and written alike by a second run with the same arguments"""
    steps, warmup = 7, 2; mine = lambda: set(glob.glob(os.path.join(tempfile.gettempdir(), "zkbench_*"))); before = mine()
    j = run(["--steps", str(steps), "--warmup", str(warmup), "--dump-outputs", str(tmp_path / "a")])
    assert {"metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"} <= set(j) and j["steps"] == steps and j["warmup"] == warmup and j["value"] > 0 and j["ms_per_step"] > 0
    assert not mine() - before, "the run left its temporary directories behind"
    assert j["full"] is False and not {"roofline", "cpu_baseline", "extra_legs", "value_from_host_buffers", "stage_ms_per_proof"} & set(j)
    p = np.load(tmp_path / "a" / "proof.npy"); assert p.dtype == np.float64 and p.shape == (8, 32) and np.array_equal(p, np.round(p)) and p.min() >= 0 and p.max() <= 255
    proof = bytes(p.astype(np.uint8).reshape(-1)).hex()
    # the statement and the randomness of the last step, as bench.py picks them: statement k = (warmup + steps - 1) mod n, (r, s) = workload.prover_rs(k), the key from its seed
    n = max(2, min(steps + warmup, 64)); k = (warmup + steps - 1) % n; d = w.send_instance(k)
    pk, vk, wp = (str(tmp_path / x) for x in ("pk.txt", "vk.txt", "w.bin"))
    e.init(); e.keygen("send", pk, vk, seed=0xB10C4A2E); e.witness_send(*[("0x" + x.hex()) if isinstance(x, bytes) else x for x in w.send_args(d)], wp)
    b = open(wp, "rb").read(); z = np.frombuffer(b, dtype=np.uint64, count=4 * int(np.frombuffer(b, dtype=np.uint64, count=1)[0]), offset=8).reshape(-1, 4)
    prover = e.Prover(pk); r, s = w.prover_rs(k); assert min(r, s).bit_length() > 240; again = prover.prove(z, r, s); prover.close()
    assert proof == again and e.verify(vk, proof, w.pack_public([d["cmtA_old"], d["sn_old"], d["cmtS"], d["cmtA"]]))
    run(["--steps", str(steps), "--warmup", str(warmup), "--dump-outputs", str(tmp_path / "b")]); assert np.array_equal(p, np.load(tmp_path / "b" / "proof.npy"))
