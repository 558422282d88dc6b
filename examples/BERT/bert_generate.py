"""Greedy continuation of a prompt with the decoder-only LM (``CausalLM.generate``: a prefill, then one KV-cache decode
step per token).

Restores the latest checkpoint of ``--ckpt_dir`` (the TensorBundle ``bert_train.py --causal`` writes; without
``--ckpt_dir`` the model keeps its random initial weights, which exercises the path and nothing else) and prints one
line of token ids per prompt: the prompt, ``|``, the continuation.

    python bert_generate.py --ckpt_dir /path/to/ckpt --prompt_ids 101,2023,2003 --new 32 [--window 256] [--eos 102]
    python bert_generate.py --tiny --prompt_len 12 --batch 2 --new 8          # generated prompts
"""
import argparse
import sys

import _path  # noqa: F401

import torch

import dtg
from dtg.models import BertConfig, CausalLM
from dtg.parallel import FlatParams


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--ckpt_dir", default=None)
    ap.add_argument("--prompt_ids", default=None, help="comma-separated token ids (one prompt)")
    ap.add_argument("--prompt_len", type=int, default=16, help="without --prompt_ids: length of the generated prompts")
    ap.add_argument("--batch", type=int, default=1, help="without --prompt_ids: number of generated prompts")
    ap.add_argument("--new", type=int, default=32, help="tokens to generate")
    ap.add_argument("--window", type=int, default=0, help="sliding window the model was trained with (0: none)")
    ap.add_argument("--eos", type=int, default=None, help="token id that ends a record")
    ap.add_argument("--prefill_chunk", type=int, default=0,
                    help="feed the prompt through attn_extend this many tokens at a time (0: the one-shot prefill)")
    ap.add_argument("--cache_dtype", choices=["bf16", "fp8"], default="bf16",
                    help="fp8: the quantised KV cache (e4m3 codes and a scale per row); bf16: the weights' dtype")
    ap.add_argument("--tiny", action="store_true", help="2-layer, 64-wide model (CPU)")
    ap.add_argument("--max_position", type=int, default=512)
    ap.add_argument("--seed", type=int, default=0)
    return ap.parse_args(argv)


def main(argv=None):
    a = parse_args(argv)
    device = torch.device("cuda" if torch.cuda.is_available() and not a.tiny else "cpu")
    cfg = BertConfig.tiny() if a.tiny else BertConfig.base()
    cfg.max_position, cfg.window = (cfg.max_position if a.tiny else a.max_position), a.window
    model = CausalLM(cfg).to(device)
    flat = FlatParams(model, compute_dtype=torch.bfloat16 if device.type == "cuda" else torch.float32)
    if a.ckpt_dir:
        prefix = dtg.train.latest_checkpoint(a.ckpt_dir)
        if prefix is None:
            print("no checkpoint in %s" % a.ckpt_dir, file=sys.stderr)
            return 1
        dtg.train.restore_flat(flat, prefix)
    if a.prompt_ids:
        ids = torch.tensor([[int(t) for t in a.prompt_ids.split(",")]], device=device)
    else:
        g = torch.Generator().manual_seed(a.seed)
        ids = torch.randint(4, min(cfg.vocab_size, 30522), (a.batch, a.prompt_len), generator=g).to(device)
    out = model.generate(ids, [ids.shape[1]] * ids.shape[0], a.new, eos_id=a.eos, prefill_chunk=a.prefill_chunk,
                         cache_dtype=torch.float8_e4m3fn if a.cache_dtype == "fp8" else None)
    for p, o in zip(ids.tolist(), out.tolist()):
        print(" ".join(map(str, p)), "|", " ".join(map(str, o)), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
