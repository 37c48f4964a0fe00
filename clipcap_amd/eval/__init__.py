"""clipcap_amd.eval — the Python surface of the reference's ``clipcap.eval`` for the metrics that need no Java jar: BLEU-1..4, ROUGE-L and
CIDEr on the device (``metrics``), ``evaluate_model`` to decode and score in one call, and ``python -m clipcap_amd.eval`` for two CSV files.
METEOR, SPICE, SPIDEr and the PTB tokenizer are out of scope."""
from clipcap_amd.eval import metrics  # noqa: F401
from clipcap_amd.eval.base import evaluate_model, run_eval  # noqa: F401
from clipcap_amd.eval.metrics import evaluate_metrics, evaluate_metrics_from_lists  # noqa: F401
