"""qldpc.misc compatibility module (reference python/qldpc/misc/__init__.py).
DemPipeline and run_dem_simulation have no reference name: they are the batched
road for a user-supplied detector error model."""
from exp_ldpc_amd.experiment import (BPDetectorCorrect, BPOSDCorrect, BPOSDCorrectSingleShot,  # noqa: F401
                                     BPOSDHybridCorrect, DemPipeline, p_sweep, p_sweep_main, run_dem_simulation,
                                     run_simulation)
from exp_ldpc_amd.experiment import add_relay_args, unpack_relay_args  # noqa: F401  (bprelay / bprelay_detector)
from exp_ldpc_amd.ldpc_compat import relay_decoder  # noqa: F401
