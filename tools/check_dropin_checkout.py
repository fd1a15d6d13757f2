"""The drop-in overlay against a checkout of the reference, by hand (needs files outside this
repository, so it is not part of the test suite):

    python tools/check_dropin_checkout.py <picotron checkout>

With the checkout on the path, the modules the overlay does not replace (pipeline engine,
checkpoint init, utils) come from the checkout and see the build's process-group global; the
reference's PipelineParallel wraps the build's Llama (train.py:174-186 order) on a 1-rank grid.
"""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CODE = """
import types, torch, torch.distributed as dist
dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%d" % __import__("random").randint(20000, 40000),
                        rank=0, world_size=1)
import picotron, picotron.process_group_manager as pgm
from picotron.pipeline_parallel.pipeline_parallel import PipelineParallel
import picotron.utils as U
import picotron.checkpoint as ck
assert PipelineParallel.__module__ == "picotron.pipeline_parallel.pipeline_parallel"
import picotron.pipeline_parallel.pipeline_parallel as PPm
import picotron_amd.pipeline_parallel.pp_communications as PC
assert PPm.pipeline_communicate is PC.pipeline_communicate
assert PPm.bidirectional_pipeline_communicate is PC.bidirectional_pipeline_communicate
assert U.pgm is pgm and ck.pgm is pgm
pgm.setup_process_group_manager(tp_size=1, cp_size=1, pp_size=1, dp_size=1)
from picotron.model import Llama
from picotron.tensor_parallel.tensor_parallel import apply_tensor_parallel
cfg = types.SimpleNamespace(hidden_size=128, intermediate_size=256, num_attention_heads=2, num_key_value_heads=2,
    vocab_size=256, rms_norm_eps=1e-5, rope_theta=10000.0, num_hidden_layers=2, max_position_embeddings=64)
m = Llama(cfg)
m = apply_tensor_parallel(m)
pp = PipelineParallel(m, cfg)
assert list(pp.decoder_layers.keys()) == ["0", "1"] and pp.final_proj is m.final_proj
print("ok")
"""


def main():
    if len(sys.argv) != 2 or not os.path.isdir(os.path.join(sys.argv[1], "picotron")):
        raise SystemExit(__doc__)
    path = [os.path.join(ROOT, "dropin"), os.path.abspath(sys.argv[1])]
    env = dict(os.environ, PYTHONPATH=os.pathsep.join(path), DEVICE="cpu", LOCAL_RANK="0")
    env.pop("PICOTRON_REFERENCE", None)
    r = subprocess.run([sys.executable, "-c", CODE], cwd=os.path.join(ROOT, "tools"), env=env, timeout=240)
    raise SystemExit(r.returncode)


if __name__ == "__main__":
    main()
