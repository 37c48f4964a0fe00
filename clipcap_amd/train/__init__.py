"""clipcap_amd.train — mirrors clipcap/train/__init__.py:1-2 (``train``, ``start_training``, ``add_training_args``), plus ``evaluate``, ``self_critical_step`` and its device-side rewards ``CiderReward`` and ``MetricReward``."""
from clipcap_amd.train.args import add_training_args  # noqa: F401
from clipcap_amd.train.train import evaluate, start_training, train  # noqa: F401
from clipcap_amd.train.self_critical import scst_tokens_and_weights, self_critical_step  # noqa: F401
from clipcap_amd.train.cider import CiderReward  # noqa: F401
from clipcap_amd.train.metrics import MetricReward  # noqa: F401
