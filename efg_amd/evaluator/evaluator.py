"""Evaluator base class and the inference loop (efg/evaluator/evaluator.py:18-60, 87-159 in minimal form)."""
from contextlib import contextmanager

import torch


class DatasetEvaluator:
    """Accumulates over (inputs, outputs) pairs with `process` and summarises with `evaluate`."""

    def reset(self):
        pass

    def process(self, inputs, outputs):
        pass

    def evaluate(self):
        pass


@contextmanager
def inference_context(model):
    """Eval mode for the duration of the block; the previous mode is restored afterwards."""
    training = model.training
    model.eval()
    try:
        yield
    finally:
        model.train(training)


def inference_on_dataset(model, data_loader, evaluator):
    """Run `model` in eval mode over `data_loader`, hand every (inputs, outputs) pair to `evaluator` and return its
    `evaluate()`.  The timing and logging of the reference loop are left out."""
    evaluator.reset()
    with inference_context(model), torch.no_grad():
        for inputs in data_loader:
            evaluator.process(inputs, model(inputs))
    return evaluator.evaluate()
