"""Training helpers (reference utils/train_utils.py).  The reference's matplotlib face grids (`vis_faces`) belong to the
encoder training, which this package does not have; only the loss aggregation the coaches use is here."""


def aggregate_loss_dict(agg_loss_dict):
    """Per-key mean over a list of loss dicts (a key missing from some dicts is averaged over those that have it)."""
    values = {}
    for output in agg_loss_dict:
        for key, value in output.items():
            values.setdefault(key, []).append(value)
    return {key: sum(v) / len(v) if v else 0 for key, v in values.items()}
