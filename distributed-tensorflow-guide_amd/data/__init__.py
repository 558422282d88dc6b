"""dtg.data -- the input pipeline: record shards, a deterministic sharded sampler, host-made augmentation parameters
and a prefetching loader (the ring of ring.py) that ends in one HIP launch per batch (ops/augment.py,
csrc/kernels/augment.hip); for token records the loader of tokens.py, on the same ring, which ends in the masking
launch (ops/mlm.py, csrc/kernels/mlm_mask.hip)."""
from .records import ShardSet, write_shard  # noqa: F401
from .sampler import ShardedSampler, EvalSampler  # noqa: F401
from .augment_params import train_params, eval_params, validate_params  # noqa: F401
from .loader import DeviceLoader, DataFeedHook  # noqa: F401
from .synthetic import (synthetic_image_set, write_image_shards, synthetic_token_set,  # noqa: F401
                        write_token_shards, check_token_fields)
from .tokens import (TokenLoader, TokenFeedHook, read_token_meta, write_token_meta, masking_args,  # noqa: F401
                     BERT_UNCASED)
